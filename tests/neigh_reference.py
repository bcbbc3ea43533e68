"""Brute-force reference of the full neighbor list (plain numpy, no GPU, no oracle).

What the device list build (kernels_neigh.hip k_build_neigh) has to produce, derived without any of its machinery: no
cells, no FP32 prefilter, no staging - every ordered pair of beads is measured in numpy.longdouble (64-bit mantissa) with
the minimum image, the special status of a pair comes from a breadth-first search over the bond graph.

A pair is UNDECIDED when its squared separation lies within `delta(box, cutneigh)` of cutneigh^2: the kernel's FP64 test
and this reference round differently there.  The inputs of every test are chosen so that there is no such pair; that is a
property of the inputs and is asserted without a GPU (test_neigh_reference_cpu.py), so a comparison never leaves a pair out.
"""
import collections

import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "numpy.longdouble has no 64-bit mantissa on this platform"


# ------------------------------------------------------------------------------------------------
# geometry
# ------------------------------------------------------------------------------------------------
def delta(box, cutneigh):
    """Half width (in r^2) of the undecided zone.  Each separation component carries at most 2^-53 * (edge + cutneigh)
    absolute error (one subtraction of the raw coordinates, one of the image shift), so r^2 of a pair at the cutoff is off
    by at most 2 * sqrt(3) * cutneigh times that plus a few ulps of r^2; 16 is a margin of ~4 over that bound."""
    box = np.asarray(box, dtype=np.float64)
    edge = float((box[:, 1] - box[:, 0]).max())
    return 16.0 * 2.0 ** -53 * cutneigh * (edge + cutneigh)


def fp32_band(box, cutneigh):
    """The FP32 error band of the list build, restated from kernels_neigh.hip rebuild_lists (`bandf`).  If that formula is
    ever narrowed, the cutoff ladder of neigh_inputs.py has to be derived again from the new one."""
    box = np.asarray(box, dtype=np.float64)
    M = float(np.abs(box).max())
    e_d = 8.0 * M * 5.97e-8
    return float(np.float32(4.0 * 1.5 * cutneigh * e_d + 3.0 * e_d * e_d + 1e-5 * cutneigh * cutneigh))


def sep2_ld(xi, xj, box):
    """Minimum-image squared separation in long double; xi, xj broadcastable float64 arrays [..., 3] (at most half a box
    outside it)."""
    box = np.asarray(box, dtype=np.float64)
    r2 = None
    for d in range(3):
        prd = LD(box[d, 1]) - LD(box[d, 0])
        half = prd / 2
        dd = np.asarray(xi[..., d], dtype=LD) - np.asarray(xj[..., d], dtype=LD)
        dd = np.where(dd > half, dd - prd, np.where(dd < -half, dd + prd, dd))
        r2 = dd * dd if r2 is None else r2 + dd * dd
    return r2


def sep2_f32(xi, xj, box):
    """r^2 the way the kernel's FP32 test (`dist2`, minimum-image variant) computes it."""
    box = np.asarray(box, dtype=np.float64)
    a, b = np.asarray(xi, dtype=np.float64).astype(np.float32), np.asarray(xj, dtype=np.float64).astype(np.float32)
    r2 = np.float32(0.0)
    for d in range(3):
        prd = box[d, 1] - box[d, 0]
        p, ip = np.float32(prd), np.float32(1.0 / prd)
        dd = a[..., d] - b[..., d]
        dd = dd - p * np.rint(dd * ip)
        r2 = r2 + dd * dd
    return r2


Reference = collections.namedtuple("Reference", "i j near_i near_j near_gap delta")


def reference_pairs(x, box, cutneigh, chunk=192):
    """All ordered pairs (i, j), i != j (0-based rows of x), with minimum-image r^2 <= cutneigh^2 in long double, by brute
    force over all N^2 candidates.  Also every candidate within 1e-3 relative of the cutoff with gap = |r^2 - cutneigh^2|."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    n = len(x)
    c2 = LD(cutneigh) * LD(cutneigh)
    near = LD(1e-3) * c2
    oi, oj, ni, nj, ng = [], [], [], [], []
    for b in range(0, n, chunk):
        e = min(n, b + chunk)
        r2 = sep2_ld(x[b:e, None, :], x[None, :, :], box)
        r2[np.arange(e - b), np.arange(b, e)] = LD(np.inf)          # i == j
        ii, jj = np.nonzero(r2 <= c2)
        oi.append(ii + b); oj.append(jj)
        gap = np.abs(r2 - c2)
        ii, jj = np.nonzero(gap <= near)
        ni.append(ii + b); nj.append(jj); ng.append(gap[ii, jj])
    cat = np.concatenate
    return Reference(cat(oi).astype(np.int64), cat(oj).astype(np.int64), cat(ni).astype(np.int64), cat(nj).astype(np.int64),
                     cat(ng), delta(box, cutneigh))


def undecided(ref):
    """Ordered candidates (i, j, gap) the comparison could not judge.  The allowed number is zero."""
    m = ref.near_gap <= LD(ref.delta)
    return list(zip(ref.near_i[m].tolist(), ref.near_j[m].tolist(), [float(g) for g in ref.near_gap[m]]))


# ------------------------------------------------------------------------------------------------
# special neighbors
# ------------------------------------------------------------------------------------------------
def reference_specials(natoms, bonds):
    """{tag: {partner tag: level}} with level 1 / 2 / 3 for 1-2 / 1-3 / 1-4 partners: breadth-first search over the bond
    graph, a partner counted at its lowest level only (the reference program's dedup).  bonds: rows (type, tag, tag)."""
    adj = [[] for _ in range(natoms + 1)]
    for row in np.asarray(bonds).reshape(-1, 3):
        a, b = int(row[1]), int(row[2])
        if a != b:
            adj[a].append(b); adj[b].append(a)
    out = {}
    for t in range(1, natoms + 1):
        if not adj[t]:
            continue
        level = {t: 0}
        frontier = [t]
        for depth in (1, 2, 3):
            nxt = []
            for u in frontier:
                for w in adj[u]:
                    if w not in level:
                        level[w] = depth
                        nxt.append(w)
            frontier = nxt
        del level[t]
        out[t] = level
    return out


def expected_code(level, lj, coul):
    """Engine::special_flag restated (src/neighbor.cpp:360-376 of the reference): None = the pair is absent from the list
    (lj and coul weight both 0); 0 = present as an ordinary entry (lj weight 1 - the engine's documented departure: the
    reference sets the level bits when only coul differs from 1, with factor 1.0); otherwise present with code = level.
    lj, coul: the three weights of `special_bonds`; level 0 = not special."""
    if level == 0:
        return 0
    if lj[level - 1] == 0.0 and coul[level - 1] == 0.0:
        return None
    if lj[level - 1] == 1.0:
        return 0
    return level


def expected_entries(ref, tags, natoms, bonds, lj, coul):
    """{(itag, jtag): code} of the full list: the reference's pairs minus the excluded specials.  tags[row] = tag of row
    `row` of the positions the reference was computed from.  (The engine, like the reference program, builds no 1-3 / 1-4
    lists when every weight from there on is 1; expected_code gives such a pair code 0 either way.)"""
    sp = reference_specials(natoms, bonds)
    tags = np.asarray(tags)
    out = {}
    for a, b in zip(tags[ref.i].tolist(), tags[ref.j].tolist()):
        lv = sp.get(a, {}).get(b, 0)
        code = expected_code(lv, lj, coul)
        if code is not None:
            out[(a, b)] = code
    return out


# ------------------------------------------------------------------------------------------------
# comparison
# ------------------------------------------------------------------------------------------------
class Report:
    def __init__(self):
        self.duplicates, self.missing, self.extra, self.wrong_code, self.asymmetric = [], [], [], [], []
        self.context = None

    @property
    def ok(self):
        return not (self.duplicates or self.missing or self.extra or self.wrong_code or self.asymmetric)

    def counts(self):
        return dict(duplicates=len(self.duplicates), missing=len(self.missing), extra=len(self.extra),
                    wrong_code=len(self.wrong_code), asymmetric=len(self.asymmetric))

    def __str__(self):
        if self.ok:
            return "neighbor list equals the reference"
        lines = ["neighbor list differs from the brute-force reference: %s" % self.counts()]
        for name in ("duplicates", "missing", "extra", "wrong_code", "asymmetric"):
            for item in getattr(self, name)[:10]:
                lines.append("  %-10s %s" % (name, describe(item, self.context)))
        return "\n".join(lines)


def describe(item, context):
    """One offending pair with the evidence a kernel author needs: tags, positions, r^2 in long double and in float32 (as
    `dist2` computes it), cutneigh^2 and the FP32 band."""
    a, b = item[0], item[1]
    text = "(%d, %d)%s" % (a, b, (" " + " ".join(str(v) for v in item[2:])) if len(item) > 2 else "")
    if context is None:
        return text
    x_by_tag, box, cutneigh = context
    xa, xb = x_by_tag[a], x_by_tag[b]
    r2 = sep2_ld(xa, xb, box)
    c2 = LD(cutneigh) * LD(cutneigh)
    return "%s x_i=%r x_j=%r r2_ld=%s r2_ld-cut2=%.3e r2_f32=%.9g cut2=%.17g band=%.3e delta=%.3e" % (
        text, xa.tolist(), xb.tolist(), np.format_float_positional(r2, precision=21), float(r2 - c2),
        float(sep2_f32(xa, xb, box)), float(c2), fp32_band(box, cutneigh), delta(box, cutneigh))


def compare(listed, expected, context=None):
    """listed: (itag, jtag, code) arrays of the list under test; expected: {(itag, jtag): code}.  context = (x_by_tag dict or
    array indexed by tag, box, cutneigh) for the failure message.  Reports, separately: duplicates in `listed`; entries
    missing; entries that should not be there; entries with the wrong code; asymmetry ((i, j) listed without (j, i), or
    with a different code)."""
    rep = Report()
    rep.context = context
    seen = {}
    for a, b, c in zip(np.asarray(listed[0]).tolist(), np.asarray(listed[1]).tolist(), np.asarray(listed[2]).tolist()):
        if (a, b) in seen:
            rep.duplicates.append((a, b, "codes %d and %d" % (seen[(a, b)], c)))
        else:
            seen[(a, b)] = c
    for key, c in seen.items():
        if key not in expected:
            rep.extra.append(key + ("code %d" % c,))
        elif expected[key] != c:
            rep.wrong_code.append(key + ("listed code %d, expected %d" % (c, expected[key]),))
        back = seen.get((key[1], key[0]))
        if back is None:
            rep.asymmetric.append(key + ("no reverse entry",))
        elif back != c:
            rep.asymmetric.append(key + ("code %d, reverse entry %d" % (c, back),))
    for key in expected:
        if key not in seen:
            rep.missing.append(key + ("expected code %d" % expected[key],))
    for name in ("duplicates", "missing", "extra", "wrong_code", "asymmetric"):
        getattr(rep, name).sort()
    return rep
