"""fix indent restated in long double: the three shapes of FixIndent::post_force with Domain::remap on the centre and
Domain::minimum_image on the difference, bead by bead.  What the fixtures' conditions, the CPU tests and the GPU tests measure
the recorded and the computed forces against; nothing here reads the engine or the reference.

An indenter is a dict: kind "sphere" | "cylinder" | "plane", K, side "in" | "out" (sphere, cylinder), dim (cylinder: the axis,
plane: the normal), ctr (three numbers; the cylinder's axis component is not used), R, and for a plane pos and planeside
(-1 lo, +1 hi)."""
import numpy as np

LD = np.longdouble


def parse(words):
    """The words of the command behind the group: K <sphere x y z R | cylinder d c1 c2 R | plane d pos lo|hi> [side in|out]
    [units box|lattice] -> indenter (numbers only)."""
    w = list(words)
    assert w[0] == "indent"
    o = dict(K=float(w[1]), side="out")
    k = 2
    while k < len(w):
        if w[k] == "sphere":
            o.update(kind="sphere", ctr=[float(v) for v in w[k + 1:k + 4]], R=float(w[k + 4]))
            k += 5
        elif w[k] == "cylinder":
            d = "xyz".index(w[k + 1])
            ctr = [0.0, 0.0, 0.0]
            others = [c for c in range(3) if c != d]
            ctr[others[0]], ctr[others[1]] = float(w[k + 2]), float(w[k + 3])
            o.update(kind="cylinder", dim=d, ctr=ctr, R=float(w[k + 4]))
            k += 5
        elif w[k] == "plane":
            o.update(kind="plane", dim="xyz".index(w[k + 1]), pos=float(w[k + 2]), planeside=-1 if w[k + 3] == "lo" else 1)
            k += 4
        elif w[k] == "side":
            o["side"] = w[k + 1]
            k += 2
        elif w[k] == "units":
            k += 2
        else:
            raise ValueError(w[k])
    return o


def remap(ctr, box):
    """Domain::remap on an orthogonal periodic box: into [lo, hi) by whole periods, one at a time as the reference adds them."""
    box = np.asarray(box, dtype=np.float64)
    out = []
    for d in range(3):
        c, lo, hi = np.float64(ctr[d]), box[d, 0], box[d, 1]
        prd = hi - lo
        while c < lo:
            c = c + prd
        while c >= hi:
            c = c - prd
        out.append(max(c, lo))
    return np.array(out, dtype=np.float64)


def minimum_image(d, box):
    """Domain::minimum_image in long double: |d| <= half a period in every dimension; also the raw difference it started from."""
    box = np.asarray(box, dtype=np.float64)
    d = np.array(d, dtype=LD)
    for c in range(3):
        prd = LD(box[c, 1]) - LD(box[c, 0])
        half = prd / 2
        for _ in range(64):
            far = np.abs(d[:, c]) > half
            if not far.any():
                break
            d[:, c] = np.where(far, np.where(d[:, c] < 0, d[:, c] + prd, d[:, c] - prd), d[:, c])
    return d


def terms(x, o, box, member=None):
    """-> dict: f (n, 3) the indenter's force on every bead, energy, findent (3) the force on the indenter, dr (n) (NaN for a
    non-member), touched (n) dr < 0, shifted (n) the minimum image differs from the raw difference."""
    x = np.asarray(x, dtype=LD)
    n = len(x)
    member = np.ones(n, dtype=bool) if member is None else np.asarray(member, dtype=bool)
    K = LD(o["K"])
    f = np.zeros((n, 3), dtype=LD)
    shifted = np.zeros(n, dtype=bool)
    if o["kind"] == "plane":
        d, ps = o["dim"], LD(o["planeside"])
        dr = ps * (LD(o["pos"]) - x[:, d])
        touched = member & (dr < 0)
        f[:, d] = np.where(touched, -ps * K * dr * dr, 0)
    else:
        ctr = remap(o["ctr"] if o["kind"] == "sphere" else [o["ctr"][c] if c != o["dim"] else np.asarray(box)[c][0] for c in range(3)], box)
        raw = x - ctr.astype(LD)[None, :]
        if o["kind"] == "cylinder":
            raw[:, o["dim"]] = 0
        del_ = minimum_image(raw, box)
        shifted = (del_ != raw).any(axis=1)
        r = np.sqrt((del_ * del_).sum(axis=1))
        R = LD(o["R"])
        dr = r - R if o["side"] == "out" else R - r
        fmag = K * dr * dr if o["side"] == "out" else -K * dr * dr
        touched = member & (dr < 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            f = np.where(touched[:, None], del_ * (fmag / r)[:, None], 0)
    energy = -(K / 3 * np.where(touched, dr, 0) ** 3).sum()
    return dict(f=f, energy=energy, findent=-f.sum(axis=0), dr=np.where(member, dr, np.nan), touched=touched, shifted=shifted & touched)
