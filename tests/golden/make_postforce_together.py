"""Records tests/golden/postforce_together_<mode>.json on an MI355X: the three runs of census_runs.together_script, each run
twice on fresh handles (the record is kept only if the two agree to the last bit), in the form of census_runs.together_pack.
The files hold the settings and the results, nothing else.  They were made with the build of the commit BEFORE the post-force
fixes got one owner (PostForce): test_gpu_postforce_together.py holds every later build to them bit for bit.
usage: python tests/golden/make_postforce_together.py [OUTDIR]      (default: this directory)"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import census_runs as cr          # noqa: E402


def main(outdir):
    os.makedirs(outdir, exist_ok=True)
    bad = 0
    for mode in cr.MODES:
        a = cr.run_together(mode, tempfile.mkdtemp())
        b = cr.run_together(mode, tempfile.mkdtemp())
        same = all(np.array_equal(a[k], b[k]) for k in ("x", "v", "f", "image", "rows", "log")) and a["stats"] == b["stats"]
        print("%-8s reproduces itself: %s; thermo rows %d, stats %s" % (mode, same, len(a["log"]), a["stats"]))
        if not same:
            bad += 1
            continue
        cr.write_record(cr.together_pack(mode, a), os.path.join(outdir, "postforce_together_%s.json" % mode))
    return bad


if __name__ == "__main__":
    sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else HERE))
