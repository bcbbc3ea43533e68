"""The long-double force reference (force_reference.py) and the inputs of the force tests (force_inputs.py), without a GPU:

  - the reference against the reference program's OWN known answers (tests/golden, unittest/force-styles/tests/*.yaml on
    data.fourmol) - it is pinned to LAMMPS without passing through the oracle;
  - its forces against the central-difference gradient of its own energy, its virials against sum r . f over its terms;
  - the FP64 oracle against it on every input, run 0 and the twelve-step trajectories: the deviations printed here are what
    the GPU bounds of test_gpu_force.py are derived from (16 x, force_compare.bound), and have to leave those bounds under the
    project's ceilings;
  - the conditions on the inputs: no pair the cutoff test could judge either way, at run 0 and in every step; every bond
    below half the shortest box edge (asserted inside the reference at every evaluation); the shapes each input is there for.
"""
import json
import os

import numpy as np
import pytest

import force_compare as fc
import force_inputs as fi
import force_reference as fr
from neigh_reference import LD, delta

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RUN0 = ["tiny", "offset", "types", "hubs", "hubs-harmonic", "angles-harmonic", "angles-cosine", "fene-large"]
RUN0_ALL = RUN0 + ["aligned"]          # (aligned: free beads only - no bonds to probe, none to cross a face)
TRAJECTORIES = [("tiny", "nve"), ("aligned", "nve"), ("offset", "nve"), ("offset", "langevin"), ("offset-pinned", "group"), ("types", "nve"),
                ("hubs", "nve"), ("hubs-harmonic", "nve"), ("angles-harmonic", "nve"), ("angles-cosine", "nve"), ("fene-large", "nve")]


# ------------------------------------------------------------------------------------------------
# the reference program's known answers
# ------------------------------------------------------------------------------------------------
def fourmol(name):
    d = json.load(open(os.path.join(G, "fourmol.json")))
    g = json.load(open(os.path.join(G, name + ".json")))
    order = np.argsort(np.array(d["tag"]))
    m = fr.Model()
    m.units, m.special_lj = "real", tuple(d["special_lj"])
    kind, style = name.split("_", 1)
    if kind == "lj":
        m.pair = dict(cut=g["cut_global"], shift=False, mix=g["mix"],
                      rows=[(int(i), int(j), e, s, g["cut_global"]) for i, j, e, s in g["pair_coeff"]])
    elif kind == "bond":
        for row in g["bond_coeff"]:
            m.bond[int(row[0])] = tuple(row[1:]) if style == "hybrid" else (style,) + tuple(row[1:])
    else:
        for row in g["angle_coeff"]:
            m.angle[int(row[0])] = (style,) + tuple(row[1:])
    S = fr.System(m, d["box"], np.array(d["type"])[order], [d["mass"][str(t + 1)] for t in range(d["ntypes"])], d["bonds"], d["angles"])
    return S, np.array(d["x"])[order], g


@pytest.mark.parametrize("name", ["lj_cut", "bond_fene", "bond_harmonic", "bond_hybrid", "angle_harmonic", "angle_cosine"])
def test_reference_reproduces_known_answers(name):
    """Initial energy, forces and stress of data.fourmol within the fixture's own epsilon (5e-14 for lj/cut, 2.5e-13 for the
    bond and angle styles; relative with floor 1 - the fixtures carry 15 - 16 digits).  data.fourmol's box is narrower than
    two cutoffs of 8: the reference sums every periodic image, as the reference program's ghost atoms do.
    Measured: lj_cut 1.3e-15 / 4.8e-15 / 6.4e-15 (energy / forces / stress), bond_hybrid 9.7e-16 / 1.0e-13 / 7.8e-14,
    angle_harmonic 7.5e-16 / 4.8e-14 / 7.6e-14."""
    S, x, g = fourmol(name)
    ev = S.evaluate(x)
    e = ev.evdwl + ev.ebond + ev.eangle
    de = float(abs(e - LD(g["init_energy"])) / abs(LD(g["init_energy"])))
    df, dv = fc.relerr(ev.f, g["init_forces"]), fc.relerr(ev.vpair + ev.vbond + ev.vangle, g["init_stress"])
    print("%s: energy %.2e forces %.2e stress %.2e (epsilon %.1e)" % (name, de, df, dv, g["epsilon"]))
    assert de < g["epsilon"] and df < g["epsilon"] and dv < g["epsilon"]
    if name == "lj_cut":
        assert S.multi_image


# ------------------------------------------------------------------------------------------------
# the reference against itself: forces = - grad E, virial trace = sum r . f
# ------------------------------------------------------------------------------------------------
H = LD("3e-5")
# Five-point stencil with h = 3e-5: the truncation error is h^4 / 30 x the fifth derivative of the energy along a coordinate
# (at most ~1e8 for 4 / r^12 at the closest contacts, r ~ 0.85: 3e-12), the rounding error is the energy of one bead's terms
# (at most ~1e3) x 2^-64 / h = 2e-12 per stencil point.  1e-10 relative with floor 1 leaves a factor of ten.
FD_BOUND = 1e-10


def probe_beads(name):
    """A handful of beads per input, chosen by what they take part in: a bead whose bond crosses a face, a hub, an angle
    vertex, the vertex of the angle hub, a free bead.  None of them in a clamped term (there the force is by design not
    the gradient of the energy) or with a pair closer than 1e-3 to a cutoff in r^2 (the stencil must not step across)."""
    case = fi.INPUTS[name]()
    S, x, v, img = fc.reference_system(name)
    ev = fc.reference_run0(name)
    banned = {t - 1 for pair in ev.fene_clamped for t in pair} | {t - 1 for tri in ev.angle_clamped for t in tri}
    want = []
    b = S.bonds
    cross = b[(img[b[:, 1] - 1] != img[b[:, 2] - 1]).any(axis=1)]
    want += [int(cross[0, 1]) - 1, int(cross[-1, 2]) - 1]
    want += [h - 1 for h in case.get("hubs", {})][:2]
    if "hub" in case:
        want += [case["hub"] - 1, case["straight"][0] - 3]
    if len(S.angles):
        a = S.angles[(img[S.angles[:, 1] - 1] != img[S.angles[:, 3] - 1]).any(axis=1)]
        want.append(int(a[0, 2]) - 1)
    want.append(S.n - 1)
    out = []
    for i in want:
        near = S.evaluate(x, only=i).gap
        if i not in banned and i not in out and near > LD("1e-3"):
            out.append(i)
    assert len(out) >= 3, (name, want, out)
    return out


@pytest.mark.parametrize("name", RUN0)
def test_forces_are_the_gradient_of_the_energy(name):
    """Measured: 3e-14 (fene-large) to 2.1e-13 (tiny)."""
    S, x, v, img = fc.reference_system(name)
    f = fc.reference_run0(name).f
    worst = 0.0
    for i in probe_beads(name):
        for d in range(3):
            e = {}
            for k in (-2, -1, 1, 2):
                xp = fr.ld(x).copy()
                xp[i, d] += k * H
                ev = S.evaluate(xp, only=i)
                e[k] = ev.evdwl + ev.ebond + ev.eangle
            grad = (e[-2] - 8 * e[-1] + 8 * e[1] - e[2]) / (12 * H)
            worst = max(worst, fc.relerr(-grad, f[i, d]))
    print("%s: max |f + dE/dx| = %.2e (relative, floor 1)" % (name, worst))
    assert worst < FD_BOUND


@pytest.mark.parametrize("name", RUN0)
def test_virial_is_the_sum_of_r_dot_f_over_the_terms(name):
    """Per contribution: the trace of the virial equals the sum over its terms of r_a . f_a over the beads a of the term, taken
    at mutually closest images (bead 2 at the origin: r_1 . f_1 for a pair or bond, r_1 . f_1 + r_3 . f_3 for an angle), the
    forces of every term add up to zero, and the per-bead forces are the sum of the per-term forces.  2^-60 relative to the
    sum of the absolute values of the products: sums of ~1e5 long-double terms (an angle's own r . f is zero - its energy does
    not change when the triple is scaled)."""
    ev = fc.reference_run0(name)
    t = ev.terms

    def close(a, b, scale):
        return abs(a - b) <= LD(2) ** -60 * scale

    for key, vir, fb in (("pair", ev.vpair, ev.f_pair), ("bond", ev.vbond, ev.f_bond)):
        if key in t:
            i, j, d, fv = t[key]
            rf = (d * fv).sum(axis=1)
            assert close(vir[0] + vir[1] + vir[2], rf.sum(), np.abs(d * fv).sum())
            acc = np.zeros_like(fb)
            for row in range(len(i)):
                acc[i[row]] += fv[row]; acc[j[row]] -= fv[row]
            assert fc.relerr(acc, fb) < 1e-17
    if "angle" in t:
        i1, i2, i3, d1, d2, f1, f3 = t["angle"]
        rf = (d1 * f1).sum(axis=1) + (d2 * f3).sum(axis=1)
        assert close(ev.vangle[0] + ev.vangle[1] + ev.vangle[2], rf.sum(), np.abs(d1 * f1).sum() + np.abs(d2 * f3).sum())
        assert len(i1) > 600
    assert fc.relerr((ev.f_pair + ev.f_bond + ev.f_angle).sum(axis=0), np.zeros(3)) < 1e-14     # Newton's third law, summed


# ------------------------------------------------------------------------------------------------
# the oracle against the reference: the figures the GPU bounds come from
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RUN0_ALL)
def test_oracle_against_reference_run0(name):
    """Measured (forces; the largest thermo keyword): tiny 2.5e-14 / 5.3e-15, offset 4.1e-14 / 8.0e-15, types 4.6e-14 / 6.9e-15,
    hubs and hubs-harmonic 2.9e-14 / 1.8e-15, angles-harmonic 5.4e-14 / 1.8e-15, angles-cosine 5.5e-14 / 1.9e-15, fene-large
    3.6e-14 / 1.5e-15, aligned 1.6e-14.  bound() fails here when 16 x a figure exceeds 1e-12: then the input is wrong."""
    dev, warnings = fc.oracle_run0(name)
    for k, v in dev.items():
        print("%s run 0: oracle deviation of %s = %.2e -> GPU bound %.2e" % (name, k, v, fc.bound(v, fc.RUN0_CEILING)))
    ev = fc.reference_run0(name)
    # the reference program prints the FENE warning from both owned ends of a bond that straddles a face (it is listed twice)
    assert warnings in (len(ev.fene_clamped), 2 * len(ev.fene_clamped))


@pytest.mark.parametrize("name,fixes", TRAJECTORIES)
def test_oracle_against_reference_trajectory(name, fixes):
    """Twelve steps (neighbor 0.2, temperature ~5): at least three list builds in the oracle, and its deviation from the
    reference after the last step.  Measured (x / v / f / thermo rows): tiny 5.7e-16 /
    5.5e-14 / 1.3e-12 / 3.1e-15; aligned 6.2e-16 / 6.3e-14 / 2.1e-12 / 1.4e-15; over the 630 - 729 bead inputs at most 3.6e-15 /
    1.1e-12 / 1.4e-11 / 5.6e-14.  Runs of 1 .. 11 steps (the states the GPU test compares in between): at most 3.0e-15 / 1.3e-12."""
    dev, builds = fc.oracle_trajectory(name, fixes)
    for k, v in dev.items():
        print("%s %s: oracle deviation of %s after %d steps = %.2e -> GPU bound %.2e" % (name, fixes, k, fc.STEPS, v, fc.bound(v, fc.TRAJ_CEILING[k])))
    assert builds >= 3, builds
    states = fc.oracle_states(name, fixes)
    for q, ceiling in fc.TRAJ_CEILING.items():
        if q in states[0]:
            worst = max(st[q] for st in states)
            print("%s %s: oracle deviation of %s after the steps 1 .. %d at most %.2e -> GPU bound %.2e" % (name, fixes, q, fc.STEPS - 1, worst, fc.bound(worst, ceiling)))


# ------------------------------------------------------------------------------------------------
# conditions on the inputs
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RUN0_ALL)
def test_no_undecided_pair_at_run0(name):
    S, x, v, img = fc.reference_system(name)
    ev = fc.reference_run0(name)
    # (delta grows with the cutoff: the largest cutoff's delta covers every type pair)
    assert float(ev.gap) > delta(S.box, S.cutmax), (ev.gap_pair, float(ev.gap))


@pytest.mark.parametrize("name,fixes", TRAJECTORIES)
def test_no_undecided_pair_in_any_step(name, fixes):
    ref = fc.reference_trajectory(name, fixes)
    need = fc.required_gap(name, fixes)
    print("%s %s: min |r^2 - cut^2| over %d evaluations = %.3e, required %.3e" % (name, fixes, len(ref["gaps"]), float(min(ref["gaps"])), need))
    assert len(ref["gaps"]) == fc.STEPS + 1 and float(min(ref["gaps"])) > need
    assert max(ref["fracs"]) < 1.0          # every bond below half the shortest box edge, every step


def test_shapes_the_inputs_are_there_for():
    import neigh_inputs
    for name in RUN0 + ["offset-pinned"]:
        S, x, v, img = fc.reference_system(name)
        b = S.bonds
        crossing = img[b[:, 1] - 1] != img[b[:, 2] - 1]
        assert crossing.any(axis=0).all(), name                     # bonds across all three pairs of faces at setup
        assert S.n % 64 != 0 and S.n <= 800, name
        assert (S.prd >= 3 * (S.cutmax + 0.4)).all(), name           # the engine's three cutoffs per edge
    # tiny: three cells per edge
    S = fc.reference_system("tiny")[0]
    assert S.n == 83 and neigh_inputs.cell_counts(S.box)[1:] == (3, 3)
    # offset: three different cell counts
    assert len(set(neigh_inputs.cell_counts(fc.reference_system("offset")[0].box))) == 3
    # types: every cutoff of the ladder in use, one pair without energy
    S = fc.reference_system("types")[0]
    assert {float(c) for c in np.unique(S.p_cut)} == {1.0, 1.12, 1.6, 1.81, 2.5} and (S.p_eps == 0).any()
    # hubs: 0 to 6 bonds per bead, a bead without neighbors, one FENE bond in the clamp, short type-2 / morse bonds
    case = fi.INPUTS["hubs"]()
    S, x, v, img = fc.reference_system("hubs")
    deg = np.bincount(S.bonds[:, 1:].ravel(), minlength=S.n + 1)[1:]
    assert set(deg.tolist()) >= {0, 1, 2, 3, 4, 5, 6}
    lone = case["lone"] - 1
    d = fr.min_image(fr.ld(x) - fr.ld(x[lone]), S.prd)
    assert np.sort(np.sqrt((d * d).sum(axis=1)))[1] > 1.12 + 0.4
    ev = fc.reference_run0("hubs")
    assert ev.fene_clamped == [case["clamped"]] == fc.reference_run0("hubs-harmonic").fene_clamped
    other = S.bonds[S.bonds[:, 0] != 1]
    d = fr.min_image(fr.ld(x[other[:, 1] - 1]) - fr.ld(x[other[:, 2] - 1]), S.prd)
    assert len(other) == 10 and np.sqrt((d * d).sum(axis=1)).max() < 0.5 * S.prd.min()
    assert {1.0, 0.3, 0.7} <= {float(w) for w in np.unique(S.w)}
    # angles: the hub in at least 12 angles, one exactly straight triple in the clamp of the harmonic style
    case = fi.INPUTS["angles-harmonic"]()
    S, x, v, img = fc.reference_system("angles-harmonic")
    assert (S.angles[:, 1:] == case["hub"]).any(axis=1).sum() >= 12
    assert fc.reference_run0("angles-harmonic").angle_clamped == [case["straight"]]
    assert (img[S.angles[:, 1] - 1] != img[S.angles[:, 3] - 1]).any(axis=0).all()          # triples straddle all three face pairs
    # aligned: in the cell order every wavefront of 64 is one zone; zone 3 is interior, zones 2 and 4 are not - and would be
    # under half the margin -, and they do have neighbors across the x face
    # - at setup and still after the twelve steps, whose three rebuilds therefore meet the same wavefronts
    S, x0, v, img = fc.reference_system("aligned")
    cut = 1.12 + 0.4
    cells = [neigh_inputs.cell_counts(S.box)[k] for k in range(3)]
    orders = []
    for x in (x0, np.asarray(fc.reference_trajectory("aligned")["xw"], dtype=np.float64)):
        c = np.floor((x - S.box[:, 0]) / (S.box[:, 1] - S.box[:, 0]) * cells).astype(int)
        order = np.lexsort((c[:, 0], c[:, 1], c[:, 2]))
        orders.append(order.reshape(5, 64))
        depth = np.minimum(x - S.box[:, 0], S.box[:, 1] - x).min(axis=1)[order].reshape(5, 64)
        assert S.n == 320 and (depth[2] > cut).all()
        for z in (1, 3):
            assert (depth[z] > 0.5 * cut).all() and (depth[z] < cut).all()
    assert all(set(orders[0][z]) == set(orders[1][z]) for z in range(5))
    x, order = x0, orders[0].ravel()
    i, j, d, fv = fc.reference_run0("aligned").terms["pair"]
    across = np.abs(x[i, 0] - x[j, 0]) > 5.0
    zone_of = np.empty(S.n, dtype=int); zone_of[order] = np.repeat(np.arange(5), 64)
    assert {1, 3} <= set(zone_of[i[across]].tolist()) | set(zone_of[j[across]].tolist())
    # the pinned beads of the group case
    S = fc.reference_system("offset-pinned", "group")[0]
    assert (~S.mobile).sum() == 90
