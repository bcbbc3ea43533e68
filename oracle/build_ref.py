"""Build the reference code into oracle/_ref/lmp (serial, no MPI / OpenMP, packages MOLECULE + MC + USER-LE).

The reference tree is configured with its own cmake, out of tree, into oracle/_ref/build; nothing is fetched and
nothing of it is copied into this repository.  `-ffp-contract=off` keeps the compiler from fusing a*b+c, so the
binary rounds every product the way the C oracle does.  oracle/_ref/ stays out of git.

    python oracle/build_ref.py [reference_dir]        (default: /root/reference)
"""
import json
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REF_DIR = os.path.join(HERE, "_ref")
LMP = os.path.join(REF_DIR, "lmp")
INFO = os.path.join(REF_DIR, "BUILD_INFO.json")
DEFAULT_REFERENCE = "/root/reference"

PACKAGES = ["MOLECULE", "MC", "USER-LE"]
CXX_FLAGS = "-O2 -ffp-contract=off"
CMAKE_FLAGS = ["-G", "Ninja", "-DCMAKE_BUILD_TYPE=Release", "-DBUILD_MPI=off", "-DBUILD_OMP=off",
               "-DWITH_JPEG=off", "-DWITH_PNG=off", "-DWITH_GZIP=off", "-DWITH_FFMPEG=off",
               "-DCMAKE_CXX_FLAGS=" + CXX_FLAGS] + ["-DPKG_%s=on" % p for p in PACKAGES]


def needed(reference=DEFAULT_REFERENCE):
    """True when the reference is present and oracle/_ref/lmp is missing or older than this recipe."""
    if not os.path.isdir(os.path.join(reference, "cmake")):
        return False
    return not os.path.isfile(LMP) or os.path.getmtime(LMP) < os.path.getmtime(os.path.abspath(__file__))


def _first_line(cmd):
    try:
        return subprocess.check_output(cmd, stderr=subprocess.STDOUT).decode().splitlines()[0].strip()
    except (OSError, subprocess.CalledProcessError, IndexError):
        return "unknown"


def build_ref(reference=DEFAULT_REFERENCE, quiet=True):
    bdir = os.path.join(REF_DIR, "build")
    os.makedirs(bdir, exist_ok=True)
    jobs = min(16, os.cpu_count() or 1)
    out = subprocess.DEVNULL if quiet else None
    subprocess.check_call(["cmake", "-S", os.path.join(reference, "cmake"), "-B", bdir] + CMAKE_FLAGS, stdout=out)
    subprocess.check_call(["cmake", "--build", bdir, "--target", "lmp", "-j", str(jobs)], stdout=out)
    shutil.copy2(os.path.join(bdir, "lmp"), LMP)
    os.utime(LMP, None)
    cxx = "c++"
    cache = os.path.join(bdir, "CMakeCache.txt")
    for ln in open(cache):
        if ln.startswith("CMAKE_CXX_COMPILER:"):
            cxx = ln.split("=", 1)[1].strip()
    info = dict(compiler=_first_line([cxx, "--version"]), cmake=_first_line(["cmake", "--version"]),
                build_type="Release", cxx_flags=CXX_FLAGS, packages=PACKAGES, mpi=False, openmp=False,
                cmake_flags=[f for f in CMAKE_FLAGS if f.startswith("-D")])
    with open(INFO, "w") as fh:
        json.dump(info, fh, indent=1, sort_keys=True)
        fh.write("\n")
    return LMP


if __name__ == "__main__":
    ref = sys.argv[1] if len(sys.argv) > 1 else DEFAULT_REFERENCE
    if not os.path.isdir(os.path.join(ref, "cmake")):
        sys.exit("build_ref: no reference tree at " + ref)
    print(build_ref(ref, quiet=False))
