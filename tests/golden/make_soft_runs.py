#!/usr/bin/env python3
"""Record the scenarios of tests/soft_runs.py with the reference binary (oracle/_ref/lmp, built by oracle/build_ref.py).

    python tests/golden/make_soft_runs.py [a | push | scenario ...]

Runs only where oracle/_ref/lmp has been built.  Writes soft_a.npz, soft_<scenario>.npz and soft_runs.json next to this file.
Only numbers are stored: parsed dump and thermo values (%.17g).  No script, log or source text of the reference goes into a
fixture.  The helpers are those of make_reference_runs.py.

(a) is refused unless soft_runs.a_conditions holds (at least 15 pairs below half their cutoff, the coincident pair, an
interacting pair at every special level); what is stored beside the recorded forces and thermo row is how far they are from the
long-double reference (soft_reference.py) - the figure the GPU bounds are 16 x of.  A (b) scenario is written only if the
reference exits 0 without ERROR, three reruns from starts moved by one ulp per coordinate build their lists on the same steps,
and soft_runs.b_conditions holds; the spread of the three reruns is what the tests take their bounds from.  (c) runs the
push-off script and lengthens the ramp until the reference's closest non-bonded pair is at least 0.85 apart.
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

import make_reference_runs as mr                # noqa: E402
import force_compare as fc                      # noqa: E402
import soft_runs as so                          # noqa: E402
from make_reference_runs import Refused         # noqa: E402
from systems import wrap_into_box               # noqa: E402

STATE = "id type x y z ix iy iz vx vy vz fx fy fz"
FMT = "thermo_modify format float %.17g\n"


def before_first_run(script, lines):
    rows = script.split("\n")
    k = next(i for i, ln in enumerate(rows) if ln.startswith("run ") or ln.startswith("run_style"))
    return "\n".join(rows[:k]) + "\n" + lines + "\n".join(rows[k:])


def state(path):
    """-> {step: rows sorted by id}"""
    out = {}
    for step, a in mr.read_dump(path).items():
        a = a[np.argsort(a[:, 0], kind="stable")]
        assert np.array_equal(a[:, 0], np.arange(1, len(a) + 1))
        out[step] = a
    return out


def make_a(work):
    os.makedirs(work, exist_ok=True)
    s, moved, same = so.soft_system(True)
    S, ev, _ = so.a_reference()
    why = so.a_conditions(S, ev, s, moved, same)
    if why:
        raise Refused("(a): " + why)
    script = before_first_run(so.a_script(), FMT) + "write_dump all custom %s/a.dump %s modify format float %%.17g sort id\n" % (work, STATE)
    text, sha = mr.run_lmp(script, s, work, "data.chain")
    rows = mr.read_thermo(text, len(so.A_THERMO))
    a = list(state(work + "/a.dump").values())[-1]
    f = a[:, 11:14]
    if rows.shape != (1, len(so.A_THERMO)) or not np.isfinite(f).all():
        raise Refused("(a): thermo rows %r" % (rows.shape,))
    th = S.thermo(ev, np.asarray(s["v"]))
    want = [th[k] for k in so.A_THERMO[1:]]
    dev = dict(f=fc.relerr(f, ev.f), rows=fc.relerr(rows[0, 1:], want))
    mr.savez_lzma(os.path.join(HERE, "soft_a.npz"), f=f, row=rows[0], start_x=a[:, 2:5])
    return dict(data_sha256=sha, beads=len(f), reference_deviation=dev, pairs=int(len(ev.terms["pair"][0])),
                conditions=so.a_counts(S, ev, s, same))


def record(scn, system, work, tag):
    os.makedirs(work, exist_ok=True)
    prefix = os.path.join(work, tag)
    last = so.last_step(scn)
    lines = ("thermo_style custom %s\n" % " ".join(so.THERMO) + FMT +
             "dump rec all custom %d %s.state %s\ndump_modify rec format float %%.17g sort id\n" % (so.STEPS, prefix, STATE))
    tail = "write_dump all custom %s.last %s modify format float %%.17g sort id\n" % (prefix, STATE)
    text, sha = mr.run_lmp(before_first_run(scn["script"], lines) + tail, system, work, "data.chain")
    st = state(prefix + ".state")
    st.update(state(prefix + ".last"))
    os.remove(prefix + ".last")
    cps = [c for c in (so.STEPS, last) if c in st]
    out = dict(thermo=mr.read_thermo(text, len(so.THERMO)), sha=sha, fene=len(re.findall("FENE bond too long", text)),
               builds=[int(v) for v in re.findall(r"Neighbor list builds = (\d+)", text)], checkpoints=sorted(set(cps)))
    out["x"] = np.array([st[c][:, 2:5] for c in out["checkpoints"]])
    out["v"] = np.array([st[c][:, 8:11] for c in out["checkpoints"]])
    out["image"] = np.array([st[c][:, 5:8].astype(np.int32) for c in out["checkpoints"]])
    out["f"] = st[out["checkpoints"][-1]][:, 11:14]
    out["start_x"] = st[0][:, 2:5]
    os.remove(prefix + ".state")
    return out


def make_scenario(scn, work):
    name = scn["name"]
    system = so.b_system()
    base = record(scn, system, os.path.join(work, name), "base")
    if not np.array_equal(base["start_x"], system["x"]):
        raise Refused("the reference's step-0 state is not the written start")
    if so.last_step(scn) not in base["checkpoints"]:
        raise Refused("no state at the last step (%r)" % base["checkpoints"])
    spread = dict(x=0.0, v=0.0, f=0.0, thermo=np.zeros_like(base["thermo"][:, 1:]))
    for d in range(mr.NPERTURB):
        run = record(scn, mr.perturbed(system, d), os.path.join(work, name), "p%d" % d)
        if run["builds"] != base["builds"] or not np.array_equal(run["image"], base["image"]) or run["thermo"].shape != base["thermo"].shape:
            raise Refused("list builds, image flags or rows changed in perturbed rerun %d" % d)
        for q in ("x", "v", "f"):
            spread[q] = max(spread[q], float(np.abs(run[q] - base[q]).max()))
        spread["thermo"] = np.maximum(spread["thermo"], np.abs(run["thermo"][:, 1:] - base["thermo"][:, 1:]))
    spread["thermo"] = spread["thermo"].tolist()
    arrays = dict(checkpoints=np.array(base["checkpoints"], dtype=np.int32), x=base["x"], v=base["v"], f=base["f"], image=base["image"],
                  thermo=base["thermo"], builds=np.array(base["builds"], dtype=np.int32), start_x=base["start_x"])
    why = so.b_conditions(arrays, scn)
    if why:
        raise Refused(why)
    mr.savez_lzma(os.path.join(HERE, "soft_%s.npz" % name), **arrays)
    return dict(data_sha256=base["sha"], fene_warnings=base["fene"], spread=spread, steps=so.last_step(scn), perturbed_reruns=mr.NPERTURB)


def make_push(work):
    os.makedirs(work, exist_ok=True)
    s = so.push_system()
    steps = 1000
    while True:
        script = (so.push_stage1(steps) + "write_dump all custom %s/s1.dump id x y z modify format float %%.17g sort id\n" % work +
                  so.PUSH_STAGE2.replace("run 200", "thermo_style custom step temp epair emol\n" + FMT + "run 200"))
        text, sha = mr.run_lmp(script, s, work, "data.chain", may_abort=True)
        ok = "ERROR" not in text
        closest = 0.0
        if ok:
            a = list(state(work + "/s1.dump").values())[-1]
            x, _ = wrap_into_box(dict(s, x=a[:, 1:4]))
            closest = so.closest_nonbonded(x, s["box"], s["bonds"])
        print("push-off over %d steps: closest pair %.4f%s" % (steps, closest, "" if ok else " (the reference ended in an error)"))
        if ok and closest >= so.PUSH_CLOSEST_REFERENCE:
            break
        steps *= 2
        if steps > 64000:
            raise Refused("push: no ramp up to 64000 steps separates the walk")
    # stage 2 in the reference: warnings after the switch to lj/cut, the last epair
    stage2 = text[text.rfind("Step"):] if "Step" in text else text
    rows = mr.read_thermo(stage2, 4)
    fene2 = len(re.findall("FENE bond too long", text.split("Loop time")[-2] if text.count("Loop time") >= 2 else text))
    control, _ = mr.run_lmp(before_first_run(so.PUSH_CONTROL, "thermo_style custom step temp epair emol\n" + FMT), s, work, "data.chain", may_abort=True)
    crow = mr.read_thermo(control, 4)
    return dict(data_sha256=sha, steps=steps, closest_after_stage1=closest, fene_warnings_stage2=fene2, epair_stage2_end=float(rows[-1, 2]),
                control_failed="ERROR" in control, control_epair=(float(crow[0, 2]) if len(crow) else None))


def main(argv):
    if not os.path.isfile(mr.LMP):
        sys.exit("make_soft_runs: build oracle/_ref/lmp first (python oracle/build_ref.py)")
    want = argv or ["a"] + so.NAMES + ["push"]
    meta_path = os.path.join(HERE, "soft_runs.json")
    meta = json.load(open(meta_path)) if (argv and os.path.exists(meta_path)) else dict(scenarios={})
    meta["build"] = json.load(open(mr.INFO))
    work = tempfile.mkdtemp(prefix="softruns_")
    failed = []
    try:
        for name in want:
            try:
                if name == "a":
                    meta["a"] = make_a(os.path.join(work, "a"))
                elif name == "push":
                    meta["push"] = make_push(os.path.join(work, "push"))
                else:
                    meta["scenarios"][name] = make_scenario(so.BY_NAME[name], work)
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
