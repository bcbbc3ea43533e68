"""fix spring/self, fix addforce and fix setforce in long double, from positions, image flags, origins and the incoming forces:
what the fixes add to (or set in) the force of every member, in the order the fixes are given, and the sums they report.
Nothing of the engine is used here, and nothing of the reference but its published definitions of the three fixes.

A fix is a dict: kind "spring" (k, dirs - a string of the letters x y z -, origin (n, 3) unwrapped), "add" (f (3,), every) or
"set" (f: three values, None for NULL); every one has `member` (n,) bool.
"""
import numpy as np

LD = np.longdouble


def unwrapped(x, image, box):
    box = np.asarray(box, dtype=LD)
    return np.asarray(x, dtype=LD) + np.asarray(image, dtype=LD) * (box[:, 1] - box[:, 0])[None, :]


def members(n, ids):
    m = np.zeros(n, dtype=bool)
    m[np.asarray(ids, dtype=np.int64) - 1] = True
    return m


def spring(k, member, origin, dirs="xyz"):
    return dict(kind="spring", k=k, member=np.asarray(member, dtype=bool), origin=np.asarray(origin, dtype=LD), dirs=dirs)


def add(f, member, every=1):
    return dict(kind="add", f=tuple(f), member=np.asarray(member, dtype=bool), every=every)


def setforce(f, member):
    return dict(kind="set", f=tuple(f), member=np.asarray(member, dtype=bool))


def apply(fixes, x, image, box, f_in, step=0):
    """-> (f_out (n, 3) long double, [per fix a dict]).  spring: energy = 0.5 k sum |d|^2 over the members, masked components
    dropped.  add: energy = -sum f . x_unwrapped, foriginal (3,) = the members' total force before the fix acted, virial (6,) =
    sum f_a x_b in the order xx yy zz xy xz yz.  set: foriginal.  A fix addforce that skips `step` (every) reports None."""
    u = unwrapped(x, image, box)
    f = np.array(f_in, dtype=LD)
    out = []
    for fx in fixes:
        m = fx["member"]
        if fx["kind"] == "spring":
            d = u - fx["origin"]
            for c, nm in enumerate("xyz"):
                if nm not in fx["dirs"]:
                    d[:, c] = 0
            d[~m] = 0
            f = f - LD(fx["k"]) * d
            out.append(dict(energy=LD(0.5) * LD(fx["k"]) * (d * d).sum()))
        elif fx["kind"] == "add":
            if step % fx.get("every", 1):
                out.append(None)
                continue
            v = np.array(fx["f"], dtype=LD)
            um = u[m]
            vir = [(v[a] * um[:, b]).sum() for a, b in ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))]
            out.append(dict(energy=-(um * v[None, :]).sum(), foriginal=f[m].sum(axis=0), virial=np.array(vir, dtype=LD)))
            f[m] = f[m] + v[None, :]
        else:
            out.append(dict(foriginal=f[m].sum(axis=0)))
            for c in range(3):
                if fx["f"][c] is not None:
                    f[m, c] = LD(fx["f"][c])
    return f, out
