"""Is the device code of two builds of a kernel file the same?  Compares two gfx950 device objects
(hipcc <the Makefile's CXXFLAGS> --cuda-device-only -c kernels_md.hip -o X.o) per kernel symbol: the same set of names,
and for each name the same code bytes and the same kernel descriptor.  Symbol order may differ between the builds, so the
descriptor's entry offset (bytes 16..23: the distance from the descriptor to the code) is left out of the comparison.
usage: compare_device_code.py BEFORE.o AFTER.o      (no GPU needed; exit status 1 on any difference)"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin") + os.sep


def kernels(obj):
    tmp = tempfile.mkdtemp()
    co = os.path.join(tmp, "co.o")
    subprocess.check_call([LLVM + "clang-offload-bundler", "--unbundle", "--type=o", "--targets=hip-amdgcn-amd-amdhsa--gfx950",
                           "--input=" + obj, "--output=" + co])
    sym = subprocess.check_output([LLVM + "llvm-readelf", "-sW", co], text=True)
    sec = subprocess.check_output([LLVM + "llvm-readelf", "-SW", co], text=True)
    secs = {}
    for m in re.finditer(r"\[\s*(\d+)\]\s+(\S+)\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", sec):
        secs[int(m.group(1))] = (m.group(2), int(m.group(3), 16), int(m.group(4), 16))
    data = open(co, "rb").read()
    out = {}
    for ln in sym.split("\n"):
        w = ln.split()
        if len(w) < 8 or w[3] not in ("FUNC", "OBJECT") or not w[6].isdigit():
            continue
        name, addr, size, ndx = w[7], int(w[1], 16), int(w[2]), int(w[6])
        if w[3] == "OBJECT" and not name.endswith(".kd"):
            continue
        _, saddr, soff = secs[ndx]
        raw = data[soff + addr - saddr: soff + addr - saddr + size]
        if name.endswith(".kd"):
            raw = raw[:16] + raw[24:]
        out[name] = (size, hashlib.sha256(raw).hexdigest())
    return out


a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
ka = {n for n in a if n + ".kd" in a}
kb = {n for n in b if n + ".kd" in b}
print("kernels: before %d, after %d; k_step: %d / %d" % (len(ka), len(kb), sum("k_step" in n for n in ka), sum("k_step" in n for n in kb)))
print("only in the first:", sorted(ka - kb)[:5], "only in the second:", sorted(kb - ka)[:5])
diff = [n for n in sorted(ka & kb) if a[n] != b[n] or a[n + ".kd"] != b[n + ".kd"]]
print("names compared: %d, differences: %d" % (len(ka & kb), len(diff)), diff[:5])
other = sorted(n for n in set(a) ^ set(b))
print("other symbols in one object only:", other[:10])
sys.exit(1 if diff or ka != kb else 0)
