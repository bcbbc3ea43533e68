#!/usr/bin/env python3
"""Record the scenarios of tests/wall_runs.py with the reference binary (oracle/_ref/lmp, built by oracle/build_ref.py).

    python tests/golden/make_wall_runs.py [a | melt | scenario ...]

Runs only where oracle/_ref/lmp has been built.  Writes wall_a_<region>.npz, wall_melt.npz, wall_b_<scenario>.npz and
wall_runs.json next to this file.  Only numbers are stored: parsed dump and thermo values (%.17g dumps).  No script, log or
source text of the reference goes into a fixture.  The helpers are those of make_reference_runs.py.

(a) is refused unless every block face and every cylinder surface has a contact, some bead has two block contacts and no bead
is outside (told from the positions, tests/wall_reference.py), and unless the wall changed the forces.  A (b) / (c) scenario is
written only if the reference exits 0 without ERROR, the bond rows of three reruns from starts moved by one ulp per coordinate
are the recorded ones at every step, and wall_runs.fixture_conditions holds: the LE fixes acted, at least 5 % of the beads are
within the wall's cutoff at the recorded step, none is outside.  The spread of the three reruns is what the tests take their
bounds from.
"""
import json
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import make_reference_runs as mr                # noqa: E402
import reference_runs as rr                     # noqa: E402
import wall_reference as wr                     # noqa: E402
import wall_runs as wl                          # noqa: E402
from make_reference_runs import Refused         # noqa: E402
from systems import wrap_into_box               # noqa: E402

DUMP = "write_dump all custom %s id fx fy fz modify format float %%.17g sort id\n"


def forces(path):
    a = list(mr.read_dump(path).values())[-1]
    assert np.array_equal(a[:, 0], np.arange(1, len(a) + 1))
    return a[:, 1:4]


def make_a(work):
    """-> meta of the (a) cases; one file per region."""
    os.makedirs(work, exist_ok=True)
    s = wl.a_system()
    fmt = lambda script: script.replace("\nrun 0\n", "\nthermo_modify format float %.17g\nrun 0\n", 1)      # noqa: E731
    base = fmt(wl.a_script(None, None, wall=False))
    text, sha = mr.run_lmp(base + DUMP % (work + "/f0.dump"), s, work, "data.chain")
    row0 = mr.read_thermo(text, 3)
    f0 = forces(work + "/f0.dump")
    worst = dict(value=0.0, case="")
    for region in wl.REGIONS:
        reg = wr.parse_region(wl.REGIONS[region].split())
        arrays = dict(f0=f0, row0=row0[0])
        for style in wl.STYLES:
            script = fmt(wl.a_script(region, style))
            script = script.replace("run 0\nfix_modify", "run 0\n" + DUMP % (work + "/f.dump") + "fix_modify")
            text, sha2 = mr.run_lmp(script, s, work, "data.chain")
            rows = mr.read_thermo(text, len(wl.A_THERMO))
            f = forces(work + "/f.dump")
            if sha2 != sha or rows.shape != (2, len(wl.A_THERMO)):
                raise Refused("(a) %s %s: thermo rows %r" % (region, style, rows.shape))
            t = wr.wall_terms(s["x"], reg, wr.parse_wall(wl.STYLES[style].split()))
            why = a_conditions(region, t, f, f0)
            if why:
                raise Refused("(a) %s %s: %s" % (region, style, why))
            # how far the long-double reference is from the recorded forces, relative to max(1, |f|)
            dev = float((np.abs((f - f0) - t["f"].astype(np.float64)) / np.maximum(1.0, np.abs(f))).max())
            if dev > worst["value"]:
                worst = dict(value=dev, case="%s %s" % (region, style))
            arrays["f_" + style], arrays["rows_" + style] = f, rows
        mr.savez_lzma(os.path.join(HERE, "wall_a_%s.npz" % region), **arrays)
    return dict(data_sha256=sha, beads=wl.A_N, reference_operation_order=worst)


def a_conditions(region, t, f, f0):
    if t["outside"].any():
        return "a bead is outside"
    if not all(h.any() for h in t["faces"]):
        return "a surface without a contact"
    if region == "block_in" and not (t["ncontact"] >= 2).any():
        return "no bead with two block contacts"
    if not np.abs(f - f0).max() > 0:
        return "the wall left the forces alone"
    return ""


def make_melt(work):
    os.makedirs(work, exist_ok=True)
    s = rr.load_melt(wl.B_N, 1, wl.B_SEED)
    # the chain as one piece: unwrapped by its image flags, in the widened box (no bond reaches through a face any more)
    old = np.asarray(s["box"], dtype=np.float64)
    s["x"] = np.asarray(s["x"]) + np.asarray(s["image"]) * (old[:, 1] - old[:, 0])[None, :]
    s["image"] = np.zeros_like(s["image"])
    s["box"] = wl.b_box()
    farthest = float(np.sqrt(((s["x"] - wl.b_centre()[None, :]) ** 2).sum(axis=1)).max())
    if farthest + 1.0 > 0.5 * (s["box"][0][1] - s["box"][0][0]):
        raise Refused("melt: the unwrapped chain does not fit the widened box")
    script = wl.b_melt_script(farthest) + "write_dump all custom %s/melt.dump id x y z ix iy iz vx vy vz modify format float %%.17g sort id\n" % work
    mr.run_lmp(script, s, work, "data.chain")
    a = list(mr.read_dump(os.path.join(work, "melt.dump")).values())[-1]
    assert np.array_equal(a[:, 0], np.arange(1, wl.B_N + 1))
    x, image = wrap_into_box(dict(s, x=a[:, 1:4], image=a[:, 4:7].astype(np.int32)))
    frac, out = wl.near_wall_fraction(x)
    if out or frac < 0.05:
        raise Refused("melt: %.3f of the beads near the wall, outside: %s" % (frac, out))
    mr.savez_lzma(os.path.join(HERE, "wall_melt.npz"), x=x, v=a[:, 7:10], image=image)
    return dict(near_wall=frac)


def record(scn, system, work, tag):
    """make_reference_runs.record for a wall scenario (its thermo columns; no angles)."""
    import re
    os.makedirs(work, exist_ok=True)
    prefix = os.path.join(work, tag)
    cps = scn["checkpoints"]
    text, sha = mr.run_lmp(wl.reference_script(scn, prefix, cps[-1]), system, work, "data.chain")
    thermo = mr.read_thermo(text, len(wl.thermo_columns(scn)))
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
        os.remove(prefix + name)
    return out


def make_scenario(scn, work):
    name = scn["name"]
    system = wl.b_system()
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
    path = os.path.join(HERE, "wall_b_%s.npz" % name)
    mr.savez_lzma(path + ".tmp", **arrays)
    fx = wl.Fixture.__new__(wl.Fixture)
    fx.name, fx.scn, fx.meta, fx.checkpoints, fx.last, fx.columns = name, scn, meta, scn["checkpoints"], last, wl.thermo_columns(scn)
    with np.load(path + ".tmp") as z:
        fx.z = {k: z[k] for k in z.files}
    why = wl.fixture_conditions(fx)
    if why:
        os.remove(path + ".tmp")
        raise Refused(why)
    meta["near_wall"] = wl.near_wall_fraction(fx.z["x"][-1], wl.group_low(fx.z["type"][-1]) if name == "group" else None)[0]
    os.replace(path + ".tmp", path)
    return meta


def main(argv):
    if not os.path.isfile(mr.LMP):
        sys.exit("make_wall_runs: build oracle/_ref/lmp first (python oracle/build_ref.py)")
    want = argv or ["a", "melt"] + wl.NAMES
    meta_path = os.path.join(HERE, "wall_runs.json")
    meta = json.load(open(meta_path)) if (argv and os.path.exists(meta_path)) else dict(scenarios={})
    meta["build"] = json.load(open(mr.INFO))
    work = tempfile.mkdtemp(prefix="wallruns_")
    failed = []
    try:
        for name in want:
            try:
                if name == "a":
                    meta["a"] = make_a(os.path.join(work, "a"))
                elif name == "melt":
                    meta["melt"] = make_melt(os.path.join(work, "melt"))
                else:
                    meta["scenarios"][name] = make_scenario(wl.BY_NAME[name], work)
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
