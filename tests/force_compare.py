"""What the force tests run on the inputs of force_inputs.py and compare: the scripts (`run 0`, and twelve steps with neighbor
0.2), the long-double reference of each (force_reference.py, computed once per process and input), the FP64 oracle's deviation
from it, and the rule that turns that deviation into the bound of a GPU test."""
import functools

import numpy as np

from force_inputs import INPUTS, script

STEPS = 12
LANGEVIN_SEED = 48611
FIXES = {"nve": "fix 1 all nve\n", "group": "group mobile type 1\nfix 1 mobile nve\n",
         "langevin": "fix 1 all nve\nfix 2 all langevin 1.0 1.0 1.0 %d\n" % LANGEVIN_SEED,
         "group-langevin": "group mobile type 1\nfix 1 mobile nve\nfix 2 all langevin 1.0 1.0 1.0 %d\n" % LANGEVIN_SEED}
THERMO_KEYS = ("evdwl", "ebond", "eangle", "pe", "ke", "temp", "press", "pxx", "pyy", "pzz", "pxy", "pxz", "pyz")
ROW_KEYS = ("temp", "epair", "emol", "etotal", "press")          # columns 1 .. 5 of the engine's thermo_history()
RUN0_CEILING = 1e-12                                             # the project's bound for single evaluations
TRAJ_CEILING = {"x": 1e-9, "v": 1e-8, "f": 1e-8, "rows": 1e-9}   # ... and for short trajectories
FLOOR = 1e-13


def relerr(a, b, floor=1.0):
    """max |a - b| / max(|a|, |b|, floor), in long double (the metric of test_gpu_md.py)."""
    from force_reference import ld
    a, b = ld(a), ld(b)
    return float((np.abs(a - b) / np.maximum(np.maximum(np.abs(a), np.abs(b)), floor)).max())


def bound(oracle_deviation, ceiling):
    """The GPU bound for a quantity: 16 x the oracle's own deviation from the reference (the kernels sum up to ~90 terms per
    bead in another order, replace divisions by reciprocals up to 1 ulp off and contract to FMAs in pair_term), at least
    1e-13, and never above the project's ceiling - an input whose FP64 rounding needs more is the wrong input."""
    b = max(16.0 * oracle_deviation, FLOOR)
    assert b <= ceiling, "16 x the oracle's deviation (%.3e) exceeds the ceiling %.1e: the input is wrong" % (oracle_deviation, ceiling)
    return b


def run0_script(name, norm=None):
    return script(INPUTS[name](), norm=norm) + "run 0\n"


def run_script(name, fixes="nve", thermo=1, steps=STEPS):
    return script(INPUTS[name](), skin="0.2") + FIXES[fixes] + "thermo %d\nrun %d\n" % (thermo, steps)


@functools.lru_cache(maxsize=None)
def reference_system(name, fixes=None):
    """(force_reference.System, x, v, image flags as read_data leaves them) of an input under its run-0 or its run script."""
    import force_reference as fr
    from systems import wrap_into_box
    s = INPUTS[name]()["system"]
    model = fr.model_from_script(run0_script(name) if fixes is None else run_script(name, fixes), s["ntypes"])
    x, img = wrap_into_box(s)
    return fr.System(model, s["box"], s["type"], s["mass"], s["bonds"], s.get("angles")), x, s["v"], img


@functools.lru_cache(maxsize=None)
def reference_run0(name):
    S, x, v, img = reference_system(name)
    return S.evaluate(x)


def thermo_of(name, ev, v, norm):
    """Reference thermo keywords of an evaluation under thermo_modify norm yes | no."""
    return reference_system(name)[0].thermo(ev, v, norm == "yes")


@functools.lru_cache(maxsize=None)
def reference_trajectory(name, fixes="nve"):
    from oracle import ranmars_stream
    S, x, v, img = reference_system(name, fixes)
    u = ranmars_stream(LANGEVIN_SEED, 3 * S.n * (STEPS + 1)) if "langevin" in fixes else None
    return S.trajectory(x, v, img, STEPS, u)


def oracle_thermo(name, o, norm):
    """The oracle's thermo keywords (its energies raw, its virial, its velocities) in the layout of THERMO_KEYS."""
    s = INPUTS[name]()["system"]
    n = len(s["x"])
    box = np.asarray(s["box"], dtype=np.float64)
    vol = float(np.prod(box[:, 1] - box[:, 0]))
    t = o.thermo()
    div = n if norm == "yes" else 1.0
    eangle = o.angle_energy()
    m = np.asarray(s["mass"])[o.types() - 1]
    v = o.v()
    k6 = [(m * v[:, a] * v[:, b]).sum() for a, b in ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))]
    out = dict(evdwl=t[6] / div, ebond=t[7] / div, eangle=eangle / div, pe=(t[6] + t[7] + eangle) / div, ke=t[5] * n / div, temp=t[0],
               press=t[4])
    out.update({k: (k6[c] + t[8 + c]) / vol for c, k in enumerate(THERMO_KEYS[7:])})
    return out


@functools.lru_cache(maxsize=None)
def oracle_run0(name):
    """{quantity: deviation of the oracle from the reference} at run 0 (thermo keywords under both norm settings), and the
    oracle's FENE warning count."""
    from systems import run_oracle
    S, x, v, img = reference_system(name)
    ev = reference_run0(name)
    o = run_oracle(run0_script(name), INPUTS[name]()["system"])
    assert np.array_equal(o.x(), x)
    dev = {"f": relerr(o.f(), ev.f)}
    for norm in ("yes", "no"):
        ref, got = thermo_of(name, ev, v, norm), oracle_thermo(name, o, norm)
        for k in THERMO_KEYS:
            dev[(k, norm)] = relerr(got[k], ref[k])
    return dev, int(o.fene_warnings())


@functools.lru_cache(maxsize=None)
def oracle_trajectory(name, fixes="nve"):
    """{x, v, f, rows: deviation of the oracle from the reference after the twelve steps (rows: over every thermo row)}, the
    oracle's list builds."""
    from systems import run_oracle
    S, x, v, img = reference_system(name, fixes)
    ref = reference_trajectory(name, fixes)
    o = run_oracle(run_script(name, fixes), INPUTS[name]()["system"])
    h = o.thermo_history()
    assert len(h) == STEPS + 1
    dev = dict(x=relerr(S.unwrapped(o.x(), o.image()), ref["x"][-1]), v=relerr(o.v(), ref["v"][-1]), f=relerr(o.f(), ref["f"]),
               rows=max(relerr(h[k, 1 + c], ref["rows"][k][key]) for k in range(STEPS + 1) for c, key in enumerate(ROW_KEYS)))
    return dev, int(o.neigh_builds())


@functools.lru_cache(maxsize=None)
def oracle_states(name, fixes="nve"):
    """[{x, v: deviation of the oracle from the reference after k steps} for k = 1 .. 11]: a fresh oracle run per k, as the
    engine is run (a run hands out its state at its end)."""
    from systems import run_oracle
    S = reference_system(name, fixes)[0]
    ref = reference_trajectory(name, fixes)
    out = []
    for k in range(1, STEPS):
        o = run_oracle(run_script(name, fixes, steps=k), INPUTS[name]()["system"])
        out.append(dict(x=relerr(S.unwrapped(o.x(), o.image()), ref["x"][k]), v=relerr(o.v(), ref["v"][k])))
    return out


def position_bound(name, fixes="nve"):
    return bound(oracle_trajectory(name, fixes)[0]["x"], TRAJ_CEILING["x"])


def required_gap(name, fixes="nve"):
    """min |r^2 - cut^2| a trajectory has to keep: 100 x (4 sqrt(3) cut tau_x) - two positions off by tau_x in every
    coordinate move r^2 of a pair at the cutoff by at most 4 sqrt(3) cut tau_x."""
    return 100.0 * 4.0 * np.sqrt(3.0) * reference_system(name, fixes)[0].cutmax * position_bound(name, fixes)
