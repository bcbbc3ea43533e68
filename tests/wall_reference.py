"""fix wall/region in long double from the textbook forms: the wall term of every bead from its position and the script's
numbers.  Shares nothing with the kernel's restatement (kernels_md.hip wall_force): the contact point is found geometrically -
the closest point of the surface (sphere, cylinder), of each face plane (block and cylinder caps seen from inside), of the
solid (block seen from outside) -, the energy is the style's formula in sigma / r, the force its derivative along the
unit vector from the contact point to the bead.

    region = dict(style="sphere", side="in", args=(xc, yc, zc, R))
             dict(style="block", side=.., args=(xlo, xhi, ylo, yhi, zlo, zhi))
             dict(style="cylinder", side="in", axis="z", args=(c1, c2, R, lo, hi))
    wall   = dict(style="lj93" | "lj126" | "lj1043" | "harmonic", epsilon=, sigma=, cutoff=)
             dict(style="morse", d0=, alpha=, r0=, cutoff=)

One deliberate departure from the textbook: for morse the reference divides the force magnitude by the distance once more
(src/fix_wall_region.cpp:403 `/ r`, then `* rinv` again in post_force); the recorded runs hold that, and so does this module.
"""
import numpy as np

LD = np.longdouble
AXES = {"x": 0, "y": 1, "z": 2}


def _energy_force(wall, r):
    """(E(r) - E(cutoff), -dE/dr) of the style, r a long-double array of contact distances."""
    r = np.asarray(r, dtype=LD)
    st, rc = wall["style"], LD(wall["cutoff"])

    def e_of(q):
        if st == "harmonic":
            return LD(wall["epsilon"]) * (rc - q) ** 2
        if st == "morse":
            d0, al, r0 = LD(wall["d0"]), LD(wall["alpha"]), LD(wall["r0"])
            return d0 * (np.exp(-2 * al * (q - r0)) - 2 * np.exp(-al * (q - r0)))
        eps, s = LD(wall["epsilon"]), LD(wall["sigma"]) / q
        if st == "lj93":
            return eps * (LD(2) / 15 * s ** 9 - s ** 3)
        if st == "lj126":
            return 4 * eps * (s ** 12 - s ** 6)
        if st == "lj1043":
            sig = LD(wall["sigma"])
            return 2 * LD(np.pi) * eps * (LD(2) / 5 * s ** 10 - s ** 4 -
                                          np.sqrt(LD(2)) * sig ** 3 / (3 * (q + LD(0.61) / np.sqrt(LD(2)) * sig) ** 3))
        raise ValueError(st)

    if st == "harmonic":
        return e_of(r), 2 * LD(wall["epsilon"]) * (rc - r)
    if st == "morse":
        d0, al, r0 = LD(wall["d0"]), LD(wall["alpha"]), LD(wall["r0"])
        f = 2 * d0 * al * (np.exp(-2 * al * (r - r0)) - np.exp(-al * (r - r0)))
        return e_of(r) - e_of(rc), f / r          # (the reference's extra 1 / r: see the module docstring)
    eps, sig, s = LD(wall["epsilon"]), LD(wall["sigma"]), LD(wall["sigma"]) / r
    if st == "lj93":
        f = eps * (LD(6) / 5 * s ** 9 - 3 * s ** 3) / r
    elif st == "lj126":
        f = 24 * eps * (2 * s ** 12 - s ** 6) / r
    else:
        f = 2 * LD(np.pi) * eps * (4 * s ** 10 / r - 4 * s ** 4 / r - np.sqrt(LD(2)) * sig ** 3 / (r + LD(0.61) / np.sqrt(LD(2)) * sig) ** 4)
    return e_of(r) - e_of(rc), f


def contact_points(x, region):
    """-> list of (point (n, 3), valid (n,)) : the surface points a bead can be in contact with, and whether that surface
    exists for the bead (a sphere's inside has none for the bead at the centre); and `matches` (n,): Region::match."""
    x = np.asarray(x, dtype=LD)
    n = len(x)
    a = [LD(v) for v in region["args"]]
    inside_wanted = region["side"] == "in"
    out = []
    if region["style"] == "sphere":
        c, R = np.array(a[:3], dtype=LD), a[3]
        d = x - c
        dist = np.sqrt((d * d).sum(axis=1))
        safe = np.where(dist > 0, dist, 1)
        out.append((c + d * (R / safe)[:, None], dist > 0))
        inside = dist <= R
    elif region["style"] == "block":
        lo, hi = np.array(a[0::2], dtype=LD), np.array(a[1::2], dtype=LD)
        inside = ((x >= lo) & (x <= hi)).all(axis=1)
        if inside_wanted:
            for dim in range(3):
                for bound in (lo, hi):
                    p = x.copy()
                    p[:, dim] = bound[dim]
                    out.append((p, np.ones(n, dtype=bool)))
        else:
            out.append((np.minimum(np.maximum(x, lo), hi), np.ones(n, dtype=bool)))
    elif region["style"] == "cylinder":
        ax = AXES[region["axis"]]
        u, w = [d for d in range(3) if d != ax]
        c1, c2, R, lo, hi = a
        d1, d2 = x[:, u] - c1, x[:, w] - c2
        rad = np.sqrt(d1 * d1 + d2 * d2)
        inside = (rad <= R) & (x[:, ax] >= lo) & (x[:, ax] <= hi)
        if not inside_wanted:
            raise ValueError("cylinder side out is not a wall of this engine")
        safe = np.where(rad > 0, rad, 1)
        p = x.copy()
        p[:, u], p[:, w] = c1 + d1 * R / safe, c2 + d2 * R / safe
        out.append((p, rad > 0))
        for bound in (lo, hi):
            p = x.copy()
            p[:, ax] = bound
            out.append((p, np.ones(n, dtype=bool)))
    else:
        raise ValueError(region["style"])
    return out, inside == inside_wanted


def wall_terms(x, region, wall, member=None):
    """-> dict f (n, 3), energy, fwall (3,) = -sum f, virial (6,) xx yy zz xy xz yz, ncontact (n,), outside (n,), all long
    double; member: boolean mask of the fix's group."""
    x = np.asarray(x, dtype=LD)
    n = len(x)
    member = np.ones(n, dtype=bool) if member is None else np.asarray(member, dtype=bool)
    points, matches = contact_points(x, region)
    f, energy, virial = np.zeros((n, 3), dtype=LD), LD(0), np.zeros(6, dtype=LD)
    ncontact, outside = np.zeros(n, dtype=np.int64), member & ~matches
    faces = []
    for p, valid in points:
        d = x - p
        r = np.sqrt((d * d).sum(axis=1))
        hit = member & matches & valid & (r < LD(wall["cutoff"]))
        outside |= hit & (r <= 0)
        hit &= r > 0
        faces.append(hit)
        if not hit.any():
            continue
        e, fm = _energy_force(wall, r[hit])
        fv = (fm / r[hit])[:, None] * d[hit]
        f[hit] += fv
        energy += e.sum()
        dh = d[hit]
        virial += np.array([(fv[:, 0] * dh[:, 0]).sum(), (fv[:, 1] * dh[:, 1]).sum(), (fv[:, 2] * dh[:, 2]).sum(),
                            (fv[:, 0] * dh[:, 1]).sum(), (fv[:, 0] * dh[:, 2]).sum(), (fv[:, 1] * dh[:, 2]).sum()], dtype=LD)
        ncontact += hit
    return dict(f=f, energy=energy, fwall=-f.sum(axis=0), virial=virial, ncontact=ncontact, outside=outside, faces=faces)


def parse_region(words):
    """The words of a `region ID style ...` line behind the ID -> the dict above."""
    style, a = words[0], list(words[1:])
    side = "in"
    if "side" in a:
        k = a.index("side")
        side = a[k + 1]
        del a[k:k + 2]
    if "units" in a:
        k = a.index("units")
        del a[k:k + 2]
    if style == "cylinder":
        return dict(style=style, side=side, axis=a[0], args=tuple(float(v) for v in a[1:6]))
    return dict(style=style, side=side, args=tuple(float(v) for v in a[:6 if style == "block" else 4]))


def parse_wall(words):
    """The words of a `fix ID group wall/region R style ...` line behind the region ID -> the dict above."""
    st, a = words[0], [float(v) for v in words[1:]]
    if st == "morse":
        return dict(style=st, d0=a[0], alpha=a[1], r0=a[2], cutoff=a[3])
    return dict(style=st, epsilon=a[0], sigma=a[1], cutoff=a[2])
