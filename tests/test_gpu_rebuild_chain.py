"""The rebuild chain under its two switches: the build-time positions kept by buffer rotation (LAMMPS_LE_NO_XHOLD_ALIAS=1
restores the copy) and the cell scan with four counts per thread (LAMMPS_LE_SCAN_TWO_PASS=1 restores the kernels with one).

Every case runs the same job in a fresh process per configuration (rebuild_chain_worker.py) - the default, and each switch
set on its own - and asserts
 (a) that x, v, image flags by tag, the build positions (xhold) and the owned tags in list order, and the pair and bond
     entries of the list in list order are BIT-IDENTICAL between the default and each switched run, after every `run`
     command: neither change touches any arithmetic, so any difference is a bug;
 (b) that the list of the last build equals the brute-force reference entry by entry, computed from the positions the
     hook reports for that build (test_gpu_neigh.check_list; for the one system above 50k beads the same long-double
     distances over candidates prefiltered in FP64, see reference_pairs_prefiltered);
 (c) that the run rebuilt several times where the case is about rebuilds inside a run.
The rotation cases use a Langevin thermostat at T = 1.5 (the 60-step run of test_gpu_neigh at T = 1 rebuilds 7 times)."""
import os
import pickle
import subprocess
import sys
import uuid

import numpy as np
import pytest

import le_state as ls
import neigh_inputs as I
import neigh_reference as R
from systems import CHAIN_SCRIPT
from test_gpu_neigh import FENE, MINIMG_SCRIPT, SHAPES, check_list

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CONFIGS = {"default": {}, "copy": {"LAMMPS_LE_NO_XHOLD_ALIAS": "1"}, "two-pass": {"LAMMPS_LE_SCAN_TWO_PASS": "1"}}
LIST_KEYS = ("owned", "xbuild", "itag", "jtag", "code", "btag", "bjtag", "btype")
STATE_KEYS = ("x", "v", "image") + LIST_KEYS + ("neigh_builds", "neigh_pairs", "rebuild_plan", "maxneigh", "special_asym")
HOT = "fix 1 all nve\nfix 2 all langevin 1.5 1.5 1.0 904297\n"
SCAN_SPAN = 4096          # cells per block of the scan (kernels_neigh.hip)


def run_job(tmp_path, label, system, actions, env, world=1):
    session = uuid.uuid4().hex[:12]
    d = os.path.join(str(tmp_path), label)
    os.makedirs(d)
    jobfile, out = os.path.join(d, "job.pkl"), os.path.join(d, "out")
    pickle.dump(dict(system=system, actions=actions), open(jobfile, "wb"))
    base = {k: v for k, v in os.environ.items() if k not in ("LAMMPS_LE_NO_XHOLD_ALIAS", "LAMMPS_LE_SCAN_TWO_PASS")}
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "rebuild_chain_worker.py"), str(r), str(world), session, jobfile, out],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=dict(base, **env)) for r in range(world)]
    logs = [p.communicate(timeout=600)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)
    return [dict(np.load("%s.r%d.npz" % (out, r))) for r in range(world)]


def twins(tmp_path, system, actions, env=None, world=1):
    """The job under every configuration; (a) for every rank and every snapshot.  Returns the default run's ranks."""
    runs = {name: run_job(tmp_path, name, system, actions, dict(env or {}, **extra), world) for name, extra in CONFIGS.items()}
    ref = runs["default"]
    for name in ("copy", "two-pass"):
        for r in range(world):
            a, b = ref[r], runs[name][r]
            assert a["snapshots"][0] == b["snapshots"][0] >= 1
            for k in range(a["snapshots"][0]):
                for key in STATE_KEYS:
                    u, v = a["s%d_%s" % (k, key)], b["s%d_%s" % (k, key)]
                    assert u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes(), \
                        "%s differs between the default and the %s run (rank %d, run command %d)" % (key, name, r, k)
    return ref


def last_list(r):
    k = r["snapshots"][0] - 1
    return {key: r["s%d_%s" % (k, key)] for key in LIST_KEYS}, k


def check_last_list(r, system, x_now=False, **kw):
    L, k = last_list(r)
    return check_list(L, system, (r["num_bond"], r["bond_type"], r["bond_atom"]), r["s%d_neigh_pairs" % k][0], FENE,
                      r["s%d_x" % k] if x_now else None, **kw)


def ncells(system):
    return int(np.prod(I.cell_counts(system["box"])))


def free_beads(pts, L):
    n = len(pts)
    return dict(box=np.array([[0.0, L]] * 3), x=np.asarray(pts, dtype=np.float64), v=np.zeros((n, 3)), type=np.ones(n, dtype=np.int32),
                mol=np.zeros(n, dtype=np.int32), image=np.zeros((n, 3), dtype=np.int32), bonds=np.zeros((0, 3), dtype=np.int32),
                ntypes=1, nbondtypes=2, mass=[1.0], extra_bond=1, extra_special=2, atom_style="bond")


# ---- the scan shapes -----------------------------------------------------------------------------------------------------
def tiny_box():
    """3 x 3 x 3 cells of edge >= cutneigh (12 x 3 x 3 of the list build's): far below one scan block."""
    rng = np.random.RandomState(31)
    s = free_beads(rng.uniform(0.0, 4.6, size=(150, 3)), 4.6)
    assert I.cell_counts(s["box"]) == (12, 3, 3)
    return s


def one_block_chain():
    s = I.translate(I.serpentine(6, 24, 24, seed=8), I.ORIGINS[2])
    assert I.cell_counts(s["box"]) == (16, 16, 16) and ncells(s) == SCAN_SPAN
    return s


def dilute_box():
    """2000 beads in groups of four, 4.27 M cells: 1042 block totals, more than the 1024 threads of a block that sums them."""
    rng = np.random.RandomState(32)
    L = 156.0
    centres = rng.uniform(1.0, L - 1.0, size=(500, 1, 3))
    s = free_beads((centres + rng.uniform(-0.5, 0.5, size=(500, 4, 3))).reshape(-1, 3), L)
    assert ncells(s) > 1024 * SCAN_SPAN and ncells(s) % SCAN_SPAN
    return s


SCAN_SHAPES = {
    "3x3x3": (tiny_box, I.ZERO_SCRIPT, "run 0\n"),
    "16x17x19-partial-last-block": (I.rebuild_chain, MINIMG_SCRIPT + HOT, "run 0\nrun 30\n"),
    "16x16x16-whole-blocks": (one_block_chain, MINIMG_SCRIPT + HOT, "run 0\nrun 30\n"),
    "cluster-in-one-cell": (I.dense_cluster, I.ZERO_SCRIPT, "run 0\n"),
    "dilute-chunked-totals": (dilute_box, I.ZERO_SCRIPT, "run 0\n"),
}


@pytest.mark.parametrize("shape", sorted(SCAN_SHAPES))
def test_scan_shapes(tmp_path, shape):
    make, head, runs = SCAN_SHAPES[shape]
    s = make()
    if shape.startswith("16x17x19"):
        assert I.cell_counts(s["box"]) == I.NONCUBIC_CELLS and SCAN_SPAN < ncells(s) < 2 * SCAN_SPAN
    (r,) = twins(tmp_path, s, [("script", head + runs)])
    if runs == "run 0\n":
        check_last_list(r, s, x_now=True)
    else:
        L0 = {key: r["s0_" + key] for key in LIST_KEYS}          # the setup build (k_wrap_bin) ...
        check_list(L0, s, (r["num_bond"], r["bond_type"], r["bond_atom"]), r["s0_neigh_pairs"][0], FENE, r["s0_x"])
        check_last_list(r, s)                                      # ... and the last one inside the run
        assert r["s1_neigh_builds"][0] >= 3


# ---- the rotation --------------------------------------------------------------------------------------------------------
RESPA = "run_style respa 3 2 3 bond 1 pair 2\n"
ROTATION = {          # name: (actions, environment)
    "thermo-7": ([("script", MINIMG_SCRIPT + HOT + "thermo 7\nrun 50\n")], {}),
    "thermo-7-energy-variant": ([("script", MINIMG_SCRIPT + HOT + "thermo 7\nrun 50\n")], SHAPES["throughput-shape"]),
    "two-runs": ([("script", MINIMG_SCRIPT + HOT + "run 25\nrun 25\n")], {}),
    "two-runs-throughput-shape": ([("script", MINIMG_SCRIPT + HOT + "run 25\nrun 25\n")], SHAPES["throughput-shape"]),
    "scatter-x-between-runs": ([("script", MINIMG_SCRIPT + HOT + "run 25\n"), ("scatter_x", 1e-3), ("script", "run 25\n")], {}),
    # right after a setup build d.pos IS the buffer that records the build: the scatter has to move d.pos off it first
    "scatter-x-after-run-0": ([("script", MINIMG_SCRIPT + HOT + "run 0\n"), ("scatter_x", 1e-3), ("snapshot", None), ("script", "run 25\n")], {}),
    "forced-regrow": ([("script", MINIMG_SCRIPT + HOT + "run 40\n")], {"LAMMPS_LE_TEST_OVERFLOW_AT": "2"}),
    "forced-regrow-throughput-shape": ([("script", MINIMG_SCRIPT + HOT + "run 40\n")],
                                       dict(SHAPES["throughput-shape"], LAMMPS_LE_TEST_OVERFLOW_AT="2")),
    "respa": ([("script", CHAIN_SCRIPT + HOT + RESPA + "thermo 20\nrun 40\n")], {}),
}


@pytest.mark.parametrize("case", sorted(ROTATION))
def test_rotation(tmp_path, case):
    """~4800 beads (four-lane look-ahead shape of the step kernel unless the case says otherwise)."""
    actions, env = ROTATION[case]
    s = I.rebuild_chain()
    (r,) = twins(tmp_path, s, actions, env)
    x, ref = check_last_list(r, s)
    k = r["snapshots"][0] - 1
    assert r["s%d_neigh_builds" % k][0] >= (3 if case != "respa" else 2)
    if case == "scatter-x-after-run-0":          # the scattered rows reached x and left the record of the build alone
        assert np.array_equal(r["s1_xbuild"], r["s0_xbuild"]) and np.array_equal(r["s1_owned"], r["s0_owned"])
        moved = np.abs(r["s1_x"] - r["s0_x"]).max(axis=1)
        assert moved.min() > 1e-5 and moved.max() <= 1.001e-3
    if case.startswith("forced-regrow"):
        assert r["s0_maxneigh"][0] > 4


def test_rotation_le_fixes_on_consecutive_steps(tmp_path):
    """The suite's `wca-fene` input (le_state.py: 600 beads, extrusion / ex_unload / ex_load fire on steps 1, 2, 3 of every 10; a
    firing that changes the topology forces a rebuild at that step), 123 steps: as many builds as the oracle counts."""
    s = ls.system_of("wca-fene")
    (r,) = twins(tmp_path, s, [("script", ls.script_of("wca-fene", 123))])
    builds = ls.oracle_end("wca-fene", 123)[0].neigh_builds()
    print("neigh_builds %d, oracle %d" % (r["s0_neigh_builds"][0], builds))
    assert r["s0_special_asym"][0] == 0 and r["s0_neigh_builds"][0] == builds >= 3
    n = len(s["x"])
    nb, bt, ba = (np.asarray(r[k]).reshape(n, -1) for k in ("num_bond", "bond_type", "bond_atom"))
    bonds = sorted({(int(bt[i, m]), min(i + 1, int(ba[i, m])), max(i + 1, int(ba[i, m]))) for i in range(n) for m in range(nb[i, 0])})
    check_last_list(r, s, bonds=np.array(bonds))


def reference_pairs_prefiltered(x, box, cutneigh, tile=4.0):
    """neigh_reference.reference_pairs for a system too large for N^2 long-double distances: the candidates are the pairs
    with an FP64 minimum-image r^2 within 2e-3 (relative) of cutneigh^2 or below - FP64 rounds r^2 by less than 1e-9 relative
    at these coordinates, so no pair of the reference or of its near band (1e-3) is lost - and each candidate gets the
    reference's own long-double distance.  The FP64 pass goes tile by tile in (y, z): the beads of a tile against every bead
    within 1.01 cutneigh of the tile (periodic)."""
    box = np.asarray(box, dtype=np.float64)
    prd = box[:, 1] - box[:, 0]
    c2 = R.LD(cutneigh) * R.LD(cutneigh)
    lim = cutneigh * cutneigh * (1.0 + 2e-3)
    nt = [max(1, int(prd[d] / tile)) for d in (1, 2)]
    edge = [prd[d] / nt[k] for k, d in enumerate((1, 2))]
    tid = [np.minimum(((x[:, d] - box[d, 0]) / edge[k]).astype(np.int64), nt[k] - 1) for k, d in enumerate((1, 2))]
    masks = []
    for k, d in enumerate((1, 2)):          # beads within reach of tile row t of dimension d
        centre = box[d, 0] + (np.arange(nt[k])[:, None] + 0.5) * edge[k]
        off = x[None, :, d] - centre
        off -= prd[d] * np.rint(off / prd[d])
        masks.append(np.abs(off) <= 0.5 * edge[k] + 1.01 * cutneigh)
    order = np.argsort(tid[1] * nt[0] + tid[0], kind="stable")
    bounds = np.searchsorted((tid[1] * nt[0] + tid[0])[order], np.arange(nt[0] * nt[1] + 1))
    ci, cj = [], []
    for t in range(nt[0] * nt[1]):
        mem = order[bounds[t]:bounds[t + 1]]
        if not len(mem):
            continue
        cand = np.nonzero(masks[0][t % nt[0]] & masks[1][t // nt[0]])[0]
        d = x[mem, None, :] - x[None, cand, :]
        d -= prd * np.rint(d / prd)
        ii, jj = np.nonzero((d * d).sum(axis=2) <= lim)
        keep = mem[ii] != cand[jj]
        ci.append(mem[ii[keep]]); cj.append(cand[jj[keep]])
    ci, cj = np.concatenate(ci), np.concatenate(cj)
    r2 = R.sep2_ld(x[ci], x[cj], box)
    inside = r2 <= c2
    gap = np.abs(r2 - c2)
    nearm = gap <= R.LD(1e-3) * c2
    return R.Reference(ci[inside].astype(np.int64), cj[inside].astype(np.int64), ci[nearm].astype(np.int64), cj[nearm].astype(np.int64),
                       gap[nearm], R.delta(box, cutneigh))


def test_rotation_above_the_four_lane_size(tmp_path):
    """50784 beads: above the 50000 up to which the step kernel takes four lanes per bead, below the 64000 up to which it loads
    ahead - the one-lane shape that reads xhold at the top of the kernel.  (Every other case here is the shape below 50k.)
    The list check is vectorised: with the FENE weights the expected entries are the reference's pairs minus the bonded ones,
    all with code 0."""
    s = I.translate(I.serpentine(6, 92, 92, seed=9), I.ORIGINS[2])
    n = len(s["x"])
    assert 50000 < n < 64000
    (r,) = twins(tmp_path, s, [("script", MINIMG_SCRIPT + HOT + "run 40\n")])
    L, k = last_list(r)
    assert r["s0_neigh_builds"][0] >= 3
    assert np.array_equal(np.sort(L["owned"]), np.arange(1, n + 1))
    x = np.empty((n, 3))
    x[L["owned"] - 1] = L["xbuild"]
    ref = reference_pairs_prefiltered(x, s["box"], I.CUTNEIGH)
    assert R.undecided(ref) == []
    key = lambda a, b: np.asarray(a, dtype=np.int64) * (n + 1) + np.asarray(b, dtype=np.int64)
    bonded = np.concatenate([key(s["bonds"][:, 1], s["bonds"][:, 2]), key(s["bonds"][:, 2], s["bonds"][:, 1])])
    expected = np.setdiff1d(key(ref.i + 1, ref.j + 1), bonded)
    listed = np.sort(key(L["itag"], L["jtag"]))
    print("pair entries %d, expected %d" % (len(listed), len(expected)))
    assert len(np.unique(listed)) == len(listed), "duplicate entries"
    assert np.array_equal(listed, expected) and not L["code"].any()
    assert np.array_equal(np.sort(key(L["btag"], L["bjtag"])), np.sort(bonded)) and (L["btype"] == 1).all()
    assert r["s0_neigh_pairs"][0] == len(listed)


# ---- decomposed runs keep the copy and the two-kernel scan -------------------------------------------------------------------
def test_decomposed_unchanged_by_the_switches(tmp_path):
    s = I.noncubic_chain(origin=1, nz=I.DD_NZ, seed=6)
    ranks = twins(tmp_path, s, [("script", CHAIN_SCRIPT + HOT + "run 30\n")], world=2)
    assert all(len(r["s0_owned"]) > 0 for r in ranks) and ranks[0]["s0_neigh_builds"][0] >= 3
    L = {key: np.concatenate([r["s0_" + key] for r in ranks]) for key in LIST_KEYS}
    r0 = ranks[0]
    check_list(L, s, (r0["num_bond"], r0["bond_type"], r0["bond_atom"]), r0["s0_neigh_pairs"][0], FENE)
