#!/usr/bin/env python3
"""Record the scenarios of tests/minimize_runs.py with the reference binary (oracle/_ref/lmp, built by oracle/build_ref.py).

    python tests/golden/make_minimize_runs.py [scenario ...]

Runs only where oracle/_ref/lmp has been built.  Writes minimize_<scenario>.npz and minimize_runs.json next to this file.  Only
numbers are stored: parsed thermo rows (%.17g), the state after the minimisation (a dump in local order, %.17g), the numbers of
the stats block with the stop string as its index, the list builds.  (No fix of these scenarios edits bonds: the bond rows
of the start are the rows at the end, and the tests hold the engine to them.)  No script, log or source text of the reference goes into a
fixture.  The helpers are those of make_reference_runs.py.

A scenario is written only if the reference exits 0 without ERROR, three reruns from starts moved by one ulp per coordinate
give the same iteration count, evaluation count, stop index, list builds, local order and image flags, and
minimize_runs.conditions holds on what would be written.  The spread of x, f, every thermo column and the stats block's
numbers over those reruns goes into minimize_runs.json; the tests take their bounds from it.
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
import minimize_runs as mn                      # noqa: E402
from make_reference_runs import Refused         # noqa: E402

STATE = "write_dump all custom %s id type x y z ix iy iz fx fy fz vx vy vz modify format float %%.17g\n"
IMAGES = "dump mni all custom 1 %s id ix iy iz\ndump_modify mni sort id\n"
BONDS = "compute mnb all property/local btype batom1 batom2\ndump mnb all local 1 %s index c_mnb[1] c_mnb[2] c_mnb[3]\n"


def record(scn, system, work, tag, images=False):
    os.makedirs(work, exist_ok=True)
    prefix = os.path.join(work, tag)
    script = mn.script(scn) + STATE % (prefix + ".state")
    if images:          # (the crossing: the image flags after every iteration; they move at list builds alone)
        script = script.replace(scn["minimize"] + "\n", IMAGES % (prefix + ".images") + scn["minimize"] + "\nundump mni\n")
    if scn["after"]:    # (then_run: the bond rows after every iteration and step, the state behind the run)
        script = script.replace(scn["minimize"] + "\n", BONDS % (prefix + ".bonds") + scn["minimize"] + "\n")
        script += scn["after"] + STATE % (prefix + ".state2")
    text, sha = mr.run_lmp(script, system, work, "data.chain")
    thermo, st = mn.parse_log(text, len(mn.columns(scn)))

    def state(path):
        a = list(mr.read_dump(path).values())[-1]
        order = a[:, 0].astype(np.int32)
        a = a[np.argsort(a[:, 0], kind="stable")]
        assert np.array_equal(a[:, 0], np.arange(1, len(a) + 1))
        os.remove(path)
        return dict(local_order=order, x=a[:, 2:5], image=a[:, 5:8].astype(np.int32), f=a[:, 8:11], v=a[:, 11:14])

    out = dict(thermo=thermo, sha=sha, st=st, **state(prefix + ".state"))
    if images:
        out["images"] = {k: b[:, 1:4].astype(np.int32) for k, b in mr.read_dump(prefix + ".images").items()}
        os.remove(prefix + ".images")
    if scn["after"]:
        out["after"] = state(prefix + ".state2")
        bonds = mr.read_dump(prefix + ".bonds")
        os.remove(prefix + ".bonds")
        out["bonds"] = {k: mr.rr.sort_rows(b[:, 1:4].astype(np.int64)).astype(np.int32) for k, b in bonds.items()}
    return out


def pick_crossing(scn, system, work):
    """Of the beads within 0.05 of a periodic face (no chain end), the one whose force at the start points through that face
    most strongly: (bead, dimension, sign).  The forces come from a minimisation of no iterations."""
    probe = record(dict(scn, before="", minimize="minimize 0 0 0 0"), system, os.path.join(work, "crossing"), "pick")
    x, f, box = np.asarray(system["x"]), probe["f"], np.asarray(system["box"])
    best = None
    for d in range(3):
        for sign, dist in ((1, box[d, 1] - x[:, d]), (-1, x[:, d] - box[d, 0])):
            push = np.where(dist < 0.05, sign * f[:, d], -np.inf)
            push[0] = push[-1] = -np.inf
            i = int(np.argmax(push))
            if best is None or push[i] > best[0]:
                best = (float(push[i]), i + 1, d, sign)
    if not best[0] > 0:
        raise Refused("no bead near a face is pushed through it")
    return dict(bead=best[1], dim=best[2], sign=best[3], push=best[0])


def make_scenario(scn, work, out=HERE):
    name = scn["name"]
    system = mn.system(scn)
    crossing = None
    if name == "crossing":
        crossing = pick_crossing(scn, system, work)
        scn = dict(scn, before=mn.crossing_before(crossing["bead"], crossing["dim"], crossing["sign"]))
    base = record(scn, system, os.path.join(work, name), "base", images=crossing is not None)
    keys = ("iterations", "evals", "stop", "builds", "steps")
    spread = dict(x=0.0, f=0.0, thermo=np.zeros_like(base["thermo"][:, 1:]), stats={k: 0.0 for k in mn.STAT_KEYS})
    for d in range(mr.NPERTURB):
        run = record(scn, mr.perturbed(system, d), os.path.join(work, name), "p%d" % d)
        if any(run["st"][k] != base["st"][k] for k in keys) or run["thermo"].shape != base["thermo"].shape:
            raise Refused("iterations, evaluations, stop or list builds changed in perturbed rerun %d: %r, not %r" %
                          (d, [run["st"][k] for k in keys], [base["st"][k] for k in keys]))
        if not (np.array_equal(run["local_order"], base["local_order"]) and np.array_equal(run["image"], base["image"])):
            raise Refused("local order or image flags changed in perturbed rerun %d" % d)
        if scn["after"]:
            a, b = run["after"], base["after"]
            if not (np.array_equal(a["local_order"], b["local_order"]) and np.array_equal(a["image"], b["image"]) and
                    sorted(run["bonds"]) == sorted(base["bonds"]) and all(np.array_equal(run["bonds"][k], base["bonds"][k]) for k in base["bonds"])):
                raise Refused("local order, image flags or bond rows of the run changed in perturbed rerun %d" % d)
            L = (np.asarray(system["box"])[:, 1] - np.asarray(system["box"])[:, 0])[None, :]
            spread["x_after"] = max(spread.get("x_after", 0.0), float(np.abs((a["x"] + a["image"] * L) - (b["x"] + b["image"] * L)).max()))
            spread["v_after"] = max(spread.get("v_after", 0.0), float(np.abs(a["v"] - b["v"]).max()))
        spread["x"] = max(spread["x"], float(np.abs(run["x"] - base["x"]).max()))
        spread["f"] = max(spread["f"], float(np.abs(run["f"] - base["f"]).max()))
        spread["thermo"] = np.maximum(spread["thermo"], np.abs(run["thermo"][:, 1:] - base["thermo"][:, 1:]))
        for k in mn.STAT_KEYS:
            spread["stats"][k] = max(spread["stats"][k], abs(float(run["st"][k]) - float(base["st"][k])))
    spread["thermo"] = spread["thermo"].tolist()
    st = base["st"]
    meta = dict(data_sha256=base["sha"], spread=spread, perturbed_reruns=mr.NPERTURB, warned=bool(st["warned"]))
    if name == "dmax_small":
        # an iteration whose search direction is the force itself (the first) ends at alphamax iff its move is dmax: a
        # one-iteration probe of the same start tells; recorded as a flag
        probe = record(dict(scn, minimize="minimize 0 0 1 10000"), system, os.path.join(work, name), "probe")
        dmax = float(scn["before"].split()[2])
        alphamax = min(1.0, dmax / probe["thermo"][0, mn.COLUMNS.index("fmax")])
        meta["alpha_is_alphamax"] = bool(probe["st"]["alpha"] == float("%.8g" % alphamax))
        meta["probe_alpha"], meta["probe_alphamax"] = probe["st"]["alpha"], alphamax
    extra = {}
    if crossing is not None:
        im, i = base["images"], crossing["bead"] - 1
        changed = [k for k in sorted(im) if k > 0 and not np.array_equal(im[k][i], im[0][i])]
        crossing["flag_changed_at"] = int(changed[0]) if changed else 0
        meta["crossing"] = crossing
    if name == "soft_overlap":
        meta["closest"] = dict(start=mn.closest_pair(system["x"], scn), end=mn.closest_pair(base["x"], scn))
    if scn["after"]:
        it = int(st["iterations"])
        steps = sorted(base["bonds"])
        first = next((k for k in steps if not np.array_equal(base["bonds"][k], base["bonds"][steps[0]])), 0)
        # an Atom::sort inside the minimisation: the local order differs from the one a minimisation of one iteration leaves
        # (its set-up sorts too; its single iteration moves nobody far enough for a list build)
        probe = record(dict(scn, minimize="minimize 0 0 1 1000", after=""), system, os.path.join(work, name), "probe")
        if probe["st"]["builds"][0] != 0:
            raise Refused("the one-iteration probe rebuilt its lists")
        meta["then_run"] = dict(first_bond_change=int(first), bonds_changed_in_min=bool(0 < first <= it),
                                sorted_inside=bool(not np.array_equal(probe["local_order"], base["local_order"])))
        a = base["after"]
        extra = dict(x_after=a["x"], v_after=a["v"], image_after=a["image"], local_order_after=a["local_order"],
                     bond_rows_min=base["bonds"][it], bond_rows_after=base["bonds"][steps[-1]])
    arrays = dict(thermo=base["thermo"], x=base["x"], f=base["f"], image=base["image"], local_order=base["local_order"],
                  builds=np.array(st["builds"], dtype=np.int32),
                  stats=np.array([float(st[k]) for k in mn.STAT_KEYS]), start_type=np.asarray(system["type"], dtype=np.int32), **extra)
    path = os.path.join(out, "minimize_%s.npz" % name)
    mr.savez_lzma(path + ".tmp", **arrays)
    fx = mn.Fixture.__new__(mn.Fixture)
    fx.name, fx.scn, fx.meta, fx.columns = name, scn, meta, mn.columns(scn)
    with np.load(path + ".tmp") as z:
        fx.z = {k: z[k] for k in z.files}
    why = mn.conditions(fx)
    if why:
        os.remove(path + ".tmp")
        raise Refused(why)
    os.replace(path + ".tmp", path)
    return meta


def main(argv, out=HERE):
    if not os.path.isfile(mr.LMP):
        sys.exit("make_minimize_runs: build oracle/_ref/lmp first (python oracle/build_ref.py)")
    want = argv or mn.NAMES
    meta_path = os.path.join(out, "minimize_runs.json")
    meta = json.load(open(meta_path)) if (argv and os.path.exists(meta_path)) else dict(scenarios={})
    meta["build"] = json.load(open(mr.INFO))
    work = tempfile.mkdtemp(prefix="minruns_")
    failed = []
    try:
        for name in want:
            try:
                meta["scenarios"][name] = make_scenario(mn.BY_NAME[name], work, out)
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
