#!/usr/bin/env python3
"""Record the scenarios of tests/reference_runs.py with the reference binary (oracle/_ref/lmp, built by oracle/build_ref.py).

    python tests/golden/make_reference_runs.py [scenario ...]

Runs only where oracle/_ref/lmp has been built.  Writes ref_melt_<key>.npz (the melted starts), ref_<scenario>.npz, ref_ranmars.npz
and ref_runs.json next to this file.  Only numbers are stored: parsed dump and thermo values.  No script, log or source text of
the reference goes into a fixture.

A scenario is written only if (a) the reference exits 0 without ERROR (FENE warnings are counted), (b) the bond and angle rows
of three reruns from starts moved by one ulp per coordinate are the recorded ones at every step, (c) every LE fix fired and
at least min_ext type-2 bonds exist at the end, (d) the scenario's own point is reached (reference_runs.reached, and the
contrast run ends elsewhere).  The spread of those three reruns is what the tests take their bounds from.

A limit scenario (reference_runs.LIMITS -> ref_limit_*.npz, the `limits` entry of ref_runs.json) is a run that is MEANT to end
in an ERROR: it is recorded with dumps after every step, flushed, and written only if the base run and the three perturbed
reruns end with the same text at the same step after the same integer rows, one kind of ERROR line appears, and the bead the
error is about sits at its limit after the last complete step (make_limit, reference_runs.limit_conditions).  Stored: the
text without its `ERROR on proc N:` prefix and `(file:line)` suffix, the step, and the state after the last complete step.
"""
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import reference_runs as rr                     # noqa: E402
import zipfile                                  # noqa: E402
from systems import write_data                  # noqa: E402

LMP = os.path.join(ROOT, "oracle", "_ref", "lmp")
INFO = os.path.join(ROOT, "oracle", "_ref", "BUILD_INFO.json")
NPERTURB = 3


class Refused(Exception):
    pass


def savez_lzma(path, **arrays):
    """make_golden.savez_lzma with a fixed time stamp on every member: the same numbers give the same file, byte for byte."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_LZMA) as z:
        for name, arr in arrays.items():
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_LZMA
            with z.open(info, "w") as fh:
                np.lib.format.write_array(fh, np.asanyarray(arr), allow_pickle=False)


def run_lmp(script, system, work, data_name, may_abort=False):
    """Write the data file, run the reference on the script; -> (log text, sha256 of the data file).  may_abort: a limit
    scenario, whose ERROR is the point (the caller reads it from the log)."""
    data = os.path.join(work, data_name)
    write_data(data, system)
    script = re.sub(r"^read_data \S+", "read_data " + data, script, flags=re.M)
    inp = os.path.join(work, "in.script")
    with open(inp, "w") as fh:
        fh.write(script)
    log = os.path.join(work, "log.out")
    rc = subprocess.call([LMP, "-in", inp, "-log", log, "-screen", "none", "-echo", "none"], cwd=work)
    text = open(log).read() if os.path.exists(log) else ""
    if (rc != 0 or "ERROR" in text) and not may_abort:
        raise Refused("(a) the reference exited %d: %s" % (rc, "; ".join(ln for ln in text.split("\n") if "ERROR" in ln)[:300]))
    return text, hashlib.sha256(open(data, "rb").read()).hexdigest()


def read_dump(path):
    """-> {step: float array (rows, columns)} of a dump custom / dump local file."""
    out, lines, i = {}, open(path).read().split("\n"), 0
    while i < len(lines):
        if lines[i].startswith("ITEM: TIMESTEP"):
            step, n = int(lines[i + 1]), int(lines[i + 3])
            i += 4
            while not (lines[i].startswith("ITEM: ATOMS") or lines[i].startswith("ITEM: ENTRIES")):
                i += 1
            rows = [ln.split() for ln in lines[i + 1:i + 1 + n]]
            if len(rows) < n or (n and len(rows[-1]) != len(rows[0])):          # (a frame the abort of a limit run cut short)
                break
            out[step] = np.array(rows, dtype=np.float64).reshape(n, -1)
            i += 1 + n
        else:
            i += 1
    return out


def read_thermo(text, ncol):
    rows = []
    for ln in text.split("\n"):
        w = ln.split()
        if len(w) == ncol and re.match(r"^\d+$", w[0]):
            try:
                rows.append([float(v) for v in w])
            except ValueError:
                pass
    return np.array(rows)


def perturbed(system, draw):
    """Every start coordinate moved by one ulp, up or down at random."""
    s = dict(system)
    rng = np.random.RandomState(1000 + draw)
    s["x"] = np.nextafter(system["x"], np.where(rng.rand(*system["x"].shape) < 0.5, -np.inf, np.inf))
    return s


def make_melt(n, nchains, seed, work):
    os.makedirs(work, exist_ok=True)
    s = rr.lattice_start(n, nchains, seed)
    script = rr.melt_script(seed) + "write_dump all custom %s/melt.dump id x y z ix iy iz vx vy vz modify format float %%.17g sort id\n" % work
    run_lmp(script, s, work, "data.chain")
    a = list(read_dump(os.path.join(work, "melt.dump")).values())[-1]
    assert np.array_equal(a[:, 0], np.arange(1, n + 1))
    # between two list builds a bead may sit just outside the box: wrap as read_data would, so that the stored start is
    # what every reader of the data file holds after reading it
    from systems import wrap_into_box
    x, image = wrap_into_box(dict(s, x=a[:, 1:4], image=a[:, 4:7].astype(np.int32)))
    savez_lzma(os.path.join(HERE, "ref_melt_%s.npz" % rr.melt_key(n, nchains, seed)), x=x, v=a[:, 7:10], image=image)


def delta_rows(by_step, last):
    """Rows of every step -> (steps at which they changed, offsets, the concatenated sorted rows)."""
    steps, offs, chunks, prev = [], [0], [], None
    for step in sorted(by_step):
        if step > last:
            break
        rows = rr.sort_rows(by_step[step][:, 1:].astype(np.int64))          # (callers pass the integer columns only)
        if prev is None or not np.array_equal(rows, prev):
            steps.append(step)
            chunks.append(rows)
            offs.append(offs[-1] + len(rows))
            prev = rows
    return np.array(steps, dtype=np.int32), np.array(offs, dtype=np.int64), np.concatenate(chunks).astype(np.int32)


def record(scn, system, work, tag):
    """One reference run of a scenario -> dict of parsed arrays."""
    os.makedirs(work, exist_ok=True)
    prefix = os.path.join(work, tag)
    cps = scn["checkpoints"]
    every = int(np.gcd.reduce(cps))
    text, sha = run_lmp(rr.reference_script(scn, prefix, every), system, work, "data.chain")
    cols = rr.thermo_columns(scn)
    thermo = read_thermo(text, len(cols))
    # (a second run prints the row of its first step again - after a velocity command with other numbers: every row is kept)
    states = read_dump(prefix + ".state")
    out = dict(thermo=thermo, sha=sha, fene=len(re.findall("FENE bond too long", text)),
               builds=[int(v) for v in re.findall(r"Neighbor list builds = (\d+)", text)])
    x, v, typ, img = [], [], [], []
    for c in cps:
        a = states[c]
        order = np.argsort(a[:, 0], kind="stable")
        local_order = a[:, 0].astype(np.int32)
        a = a[order]
        assert np.array_equal(a[:, 0], np.arange(1, len(a) + 1))
        typ.append(a[:, 1].astype(np.int32)), x.append(a[:, 2:5]), img.append(a[:, 5:8].astype(np.int32)), v.append(a[:, 8:11])
        f = a[:, 11:14]
    out.update(x=np.array(x), v=np.array(v), type=np.array(typ), image=np.array(img), f=f, local_order=local_order)
    start = states[0][np.argsort(states[0][:, 0], kind="stable")]
    out["start_x"], out["start_image"] = start[:, 2:5], start[:, 5:8].astype(np.int32)
    bonds = read_dump(prefix + ".bonds")          # index, type, atom1, atom2, length
    out["longest"] = max([float(a[a[:, 1] == 2, 4].max()) for s, a in bonds.items() if s <= cps[-1] and (a[:, 1] == 2).any()] + [0.0])
    out["bond"] = delta_rows({s: a[:, :4] for s, a in bonds.items()}, cps[-1])
    if rr.has_angles(scn):
        out["angle"] = delta_rows(read_dump(prefix + ".angles"), cps[-1])
    if scn.get("limit"):
        a = read_dump(prefix + ".nbonds")[cps[-1]]
        out["num_bond"] = a[np.argsort(a[:, 0], kind="stable"), 1].astype(np.int32)
    for name in (".state", ".bonds", ".angles", ".nbonds"):
        if os.path.exists(prefix + name):
            os.remove(prefix + name)
    return out


def same_rows(a, b):
    return all(np.array_equal(p, q) for p, q in zip(a, b))


def box_lengths(system):
    return (np.asarray(system["box"])[:, 1] - np.asarray(system["box"])[:, 0])[None, :]


def make_scenario(scn, work, melts, out=HERE):
    name = scn["name"]
    p = scn["system"]
    key = (p["n"], p.get("nchains", 1), p.get("seed", 1))
    system = rr.build_system(scn, melt=melts(*key))
    base = record(scn, system, os.path.join(work, name), "base")
    L = box_lengths(system)
    # the reference read the start we wrote: coordinates bit for bit (they lie inside the box), image flags too
    if not (np.array_equal(base["start_x"], system["x"]) and np.array_equal(base["start_image"], system["image"])):
        raise Refused("the reference's step-0 state is not the written start")
    cps = scn["checkpoints"]
    spread = dict(x={}, v={}, f={}, thermo=np.zeros_like(base["thermo"][:, 1:]))
    for d in range(NPERTURB):
        run = record(scn, perturbed(system, d), os.path.join(work, name), "p%d" % d)
        if not same_rows(run["bond"], base["bond"]) or ("angle" in base and not same_rows(run["angle"], base["angle"])):
            raise Refused("(b) bond or angle rows changed in perturbed rerun %d" % d)
        if not (np.array_equal(run["type"], base["type"]) and np.array_equal(run["image"], base["image"]) and
                run["builds"] == base["builds"] and np.array_equal(run["local_order"], base["local_order"])):
            raise Refused("(b) types, image flags, list builds or local order changed in perturbed rerun %d" % d)
        for k, c in enumerate(cps):
            ux = (run["x"][k] + run["image"][k] * L) - (base["x"][k] + base["image"][k] * L)
            spread["x"][str(c)] = max(spread["x"].get(str(c), 0.0), float(np.abs(ux).max()))
            spread["v"][str(c)] = max(spread["v"].get(str(c), 0.0), float(np.abs(run["v"][k] - base["v"][k]).max()))
        spread["f"][str(cps[-1])] = max(spread["f"].get(str(cps[-1]), 0.0), float(np.abs(run["f"] - base["f"]).max()))
        spread["thermo"] = np.maximum(spread["thermo"], np.abs(run["thermo"][:, 1:] - base["thermo"][:, 1:]))
    spread["thermo"] = spread["thermo"].tolist()
    contrast_differs = None
    if scn["contrast"]:
        old, new = scn["contrast"]
        assert scn["script"].count(old) == 1, (name, old)
        other = dict(scn, script=scn["script"].replace(old, new))
        alt = record(other, system, os.path.join(work, name), "contrast")
        contrast_differs = bool(not same_rows(alt["bond"], base["bond"]) or not np.array_equal(alt["x"][-1], base["x"][-1]))
    arrays = dict(checkpoints=np.array(cps, dtype=np.int32), x=base["x"], v=base["v"], f=base["f"], type=base["type"],
                  image=base["image"], thermo=base["thermo"], local_order=base["local_order"],
                  bond_steps=base["bond"][0], bond_offsets=base["bond"][1], bond_rows=base["bond"][2],
                  builds=np.array(base["builds"], dtype=np.int32), start_type=np.asarray(system["type"], dtype=np.int32))
    if "file_order" in system:
        arrays["start_file_order"] = np.asarray(system["file_order"], dtype=np.int32)
    if "angle" in base:
        arrays.update(angle_steps=base["angle"][0], angle_offsets=base["angle"][1], angle_rows=base["angle"][2])
    if "num_bond" in base:
        arrays["num_bond"] = base["num_bond"]
    meta = dict(data_sha256=base["sha"], fene_warnings=base["fene"], spread=spread, contrast_differs=contrast_differs,
                steps=cps[-1], perturbed_reruns=NPERTURB, perturbed_rows_identical=True, longest_extruder_bond=base["longest"])
    # (c), (d) on what would be written
    path = os.path.join(out, "ref_%s.npz" % name)
    tmp = path + ".tmp"
    savez_lzma(tmp, **arrays)
    fx = rr.Fixture.__new__(rr.Fixture)
    fx.name, fx.scn, fx.meta, fx.checkpoints, fx.last, fx.columns = name, scn, meta, cps, cps[-1], rr.thermo_columns(scn)
    with np.load(tmp) as z:
        fx.z = {k: z[k] for k in z.files}
    fx.system = lambda: system
    fx.error = fx.error_step = None
    why = rr.limit_conditions(fx) if scn.get("limit") else rr.fixture_conditions(fx)
    if why:
        os.remove(tmp)
        raise Refused(why)
    os.replace(tmp, path)
    return meta


# ------------------------------------------------------------------------------------------------------------------
# limit scenarios: the reference is meant to abort
# ------------------------------------------------------------------------------------------------------------------
ERROR_LINE = re.compile(r"^ERROR(?: on proc \d+)?: (.*?)(?: \(\S+:\d+\))?\s*$", re.M)


def record_limit(scn, system, work, tag):
    """One reference run of a limit scenario (dumps after every step, flushed) -> what survived the abort: the error text
    without its `ERROR on proc N:` prefix and `(file:line)` suffix, the last complete step S, the state and rows up to S."""
    os.makedirs(work, exist_ok=True)
    prefix = os.path.join(work, tag)
    text, sha = run_lmp(rr.reference_script(scn, prefix, 1), system, work, "data.chain", may_abort=True)
    errors = ERROR_LINE.findall(text)
    if not errors:
        raise Refused("the reference ran to the end: no ERROR")
    states, bonds, counts = read_dump(prefix + ".state"), read_dump(prefix + ".bonds"), read_dump(prefix + ".nbonds")
    angles = read_dump(prefix + ".angles") if rr.has_angles(scn) else None
    thermo = read_thermo(text, len(rr.thermo_columns(scn)))
    last = min(max(states), max(bonds), max(counts), int(thermo[-1, 0]), *([max(angles)] if angles else []))
    a = states[last]
    local_order = a[:, 0].astype(np.int32)
    a = a[np.argsort(a[:, 0], kind="stable")]
    assert np.array_equal(a[:, 0], np.arange(1, len(a) + 1))
    c = counts[last]
    start = states[0][np.argsort(states[0][:, 0], kind="stable")]
    out = dict(errors=errors, last=last, sha=sha, fene=len(re.findall("FENE bond too long", text)), thermo=thermo[thermo[:, 0] == last][-1:],
               type=a[:, 1].astype(np.int32), x=a[:, 2:5], image=a[:, 5:8].astype(np.int32), v=a[:, 8:11], local_order=local_order,
               num_bond=c[np.argsort(c[:, 0], kind="stable"), 1].astype(np.int32), start_x=start[:, 2:5],
               start_image=start[:, 5:8].astype(np.int32), bond=delta_rows({s: b[:, :4] for s, b in bonds.items()}, last))
    if angles:
        out["angle"] = delta_rows(angles, last)
    for name in (".state", ".bonds", ".angles", ".nbonds"):
        if os.path.exists(prefix + name):
            os.remove(prefix + name)
    return out


def make_limit(scn, work, melts, out=HERE):
    """A limit scenario is written only if the base run and the three perturbed reruns end with the same text at the same
    step and with the same integer rows before it, exactly one kind of ERROR line appears, and the bead the error is about
    sits at its limit after the last complete step (reference_runs.limit_conditions)."""
    if scn["runs_on"]:
        return make_scenario(scn, work, melts, out)
    name, p = scn["name"], scn["system"]
    system = rr.build_system(scn, melt=melts(p["n"], p.get("nchains", 1), p.get("seed", 1)))
    base = record_limit(scn, system, os.path.join(work, name), "base")
    if not (np.array_equal(base["start_x"], system["x"]) and np.array_equal(base["start_image"], system["image"])):
        raise Refused("the reference's step-0 state is not the written start")
    last, L = base["last"], box_lengths(system)
    spread = dict(x={str(last): 0.0}, v={str(last): 0.0}, thermo=np.zeros_like(base["thermo"][:, 1:]))
    for d in range(NPERTURB):
        run = record_limit(scn, perturbed(system, d), os.path.join(work, name), "p%d" % d)
        if run["errors"] != base["errors"] or run["last"] != last:
            raise Refused("(b) perturbed rerun %d ends with %r after step %d, not %r after step %d" % (d, run["errors"], run["last"], base["errors"], last))
        if not same_rows(run["bond"], base["bond"]) or ("angle" in base and not same_rows(run["angle"], base["angle"])):
            raise Refused("(b) bond or angle rows changed in perturbed rerun %d" % d)
        if not all(np.array_equal(run[k], base[k]) for k in ("type", "image", "local_order", "num_bond")):
            raise Refused("(b) types, image flags, bond counts or local order changed in perturbed rerun %d" % d)
        ux = (run["x"] + run["image"] * L) - (base["x"] + base["image"] * L)
        spread["x"][str(last)] = max(spread["x"][str(last)], float(np.abs(ux).max()))
        spread["v"][str(last)] = max(spread["v"][str(last)], float(np.abs(run["v"] - base["v"]).max()))
        spread["thermo"] = np.maximum(spread["thermo"], np.abs(run["thermo"][:, 1:] - base["thermo"][:, 1:]))
    spread["thermo"] = spread["thermo"].tolist()
    arrays = dict(checkpoints=np.array([last], dtype=np.int32), thermo=base["thermo"], local_order=base["local_order"],
                  num_bond=base["num_bond"], bond_steps=base["bond"][0], bond_offsets=base["bond"][1], bond_rows=base["bond"][2],
                  start_type=np.asarray(system["type"], dtype=np.int32))
    if last > 0:          # (after step 0 the state is the start itself, compared above)
        arrays.update(x=base["x"][None], v=base["v"][None], type=base["type"][None], image=base["image"][None])
    if "angle" in base:
        arrays.update(angle_steps=base["angle"][0], angle_offsets=base["angle"][1], angle_rows=base["angle"][2])
    meta = dict(error=base["errors"][0], error_step=last + 1, error_kinds=len(set(base["errors"])), data_sha256=base["sha"],
                fene_warnings=base["fene"], spread=spread, steps=last, perturbed_reruns=NPERTURB, perturbed_same_error=True,
                perturbed_rows_identical=True)
    path = os.path.join(out, "ref_%s.npz" % name)
    tmp = path + ".tmp"
    savez_lzma(tmp, **arrays)
    fx = rr.Fixture.__new__(rr.Fixture)
    fx.name, fx.scn, fx.meta, fx.checkpoints, fx.last, fx.columns = name, scn, meta, [last], last, rr.thermo_columns(scn)
    fx.error, fx.error_step = meta["error"], meta["error_step"]
    with np.load(tmp) as z:
        fx.z = {k: z[k] for k in z.files}
    fx.system = lambda: system
    why = rr.limit_conditions(fx)
    if why:
        os.remove(tmp)
        raise Refused(why)
    os.replace(tmp, path)
    return meta


def make_ranmars(work):
    os.makedirs(work, exist_ok=True)
    s, arrays, worst = rr.ranmars_system(), {}, 0.0
    for seed in rr.RANMARS_SEEDS:
        script = rr.ranmars_script(seed)
        for k in range(rr.RANMARS_RUNS):
            script += "run 0\nwrite_dump all custom %s/f%d.dump id fx fy fz modify format float %%.17g sort id\n" % (work, k)
        run_lmp(script, s, work, "data.chain")
        f = [list(read_dump("%s/f%d.dump" % (work, k)).values())[0][:, 1:4] for k in range(rr.RANMARS_RUNS)]
        draws, off = rr.draws_from_forces(np.concatenate(f))
        worst = max(worst, off)
        arrays["seed_%d" % seed] = draws.astype(np.int32)
    if worst > 1e-8:
        raise Refused("RanMars read-out is %.2e off an integer" % worst)
    savez_lzma(os.path.join(HERE, "ref_ranmars.npz"), **arrays)
    return dict(draws_per_seed=3 * rr.RANMARS_BEADS * rr.RANMARS_RUNS, worst_offset_from_integer=worst)


def main(argv):
    if not os.path.isfile(LMP):
        sys.exit("make_reference_runs: build oracle/_ref/lmp first (python oracle/build_ref.py)")
    want = argv or rr.NAMES + rr.LIMIT_NAMES + ["ranmars"]          # (twins before the limit scenarios that name them)
    meta_path = os.path.join(HERE, "ref_runs.json")
    meta = json.load(open(meta_path)) if (argv and os.path.exists(meta_path)) else dict(scenarios={})
    meta.setdefault("limits", {})
    meta["build"] = json.load(open(INFO))
    meta["factor"] = rr.FACTOR
    work = tempfile.mkdtemp(prefix="refruns_")
    made = set()

    def melts(n, nchains, seed):
        key = rr.melt_key(n, nchains, seed)
        if key not in made:
            make_melt(n, nchains, seed, os.path.join(work, "melt_" + key))
            made.add(key)
        return rr.load_melt(n, nchains, seed)

    failed = []
    try:
        for name in want:
            try:
                if name == "ranmars":
                    meta["ranmars"] = make_ranmars(os.path.join(work, "ranmars"))
                elif name in rr.LIMIT_BY_NAME:
                    meta["limits"][name] = make_limit(rr.LIMIT_BY_NAME[name], work, melts)
                else:
                    meta["scenarios"][name] = make_scenario(rr.BY_NAME[name], work, melts)
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
