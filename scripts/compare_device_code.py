"""Is the device code of two builds of a kernel file the same?  Compares two gfx950 device objects
(hipcc <the Makefile's CXXFLAGS> --cuda-device-only -c kernels_md.hip -o X.o) per kernel symbol: the same set of names,
and for each name the same code bytes and the same kernel descriptor.  Symbol order may differ between the builds, so the
descriptor's entry offset (bytes 16..23: the distance from the descriptor to the code) is left out of the comparison.
usage: compare_device_code.py [--renamed | --step-keys] BEFORE.o AFTER.o      (no GPU needed; exit status 1 on any difference)
--step-keys: for the change of k_step's fifteen template arguments into one key - every k_step<fifteen arguments> of the first
object is paired BY NAME with k_step<the key of those arguments> of the second and must have the same code bytes and the same
whole descriptor; a kernel of either object that is left without a partner fails.  (--renamed accepts any twin; this pins the
bit order.)
--renamed: for a change that adds template or kernel arguments to a kernel, which renames every instantiation - a kernel whose
name is in the first object only passes if some kernel whose name is in the second object only has the same code bytes and
the same descriptor but for its kernarg size (bytes 8..11).  Kernels in both objects are compared by name as always."""
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
        out[name] = (size, hashlib.sha256(raw).hexdigest(), hashlib.sha256(raw[:8] + raw[12:]).hexdigest() if name.endswith(".kd") else "")
    return out


def step_key(symbol):
    """The key of a k_step symbol: k_step<KEY> names it; of k_step<L, N, I, P, LPB, ...> - fifteen arguments - it is argument b
    as bit b, the lanes per bead (argument 4, 1 | 4) as `== 4` (csrc/step_plan.h, StepKeyBit).  None: not a k_step symbol."""
    m = re.search(r"6k_stepI((?:L[bi]\d+E)+)E", symbol)
    if not m:
        return None
    v = [int(x) for x in re.findall(r"L[bi](\d+)E", m.group(1))]
    if len(v) == 1:
        return v[0]
    assert len(v) == 15 and v[4] in (1, 4), symbol
    return sum((x == 4 if b == 4 else x != 0) << b for b, x in enumerate(v))


renamed = "--renamed" in sys.argv[1:]
step_keys = "--step-keys" in sys.argv[1:]
args = [x for x in sys.argv[1:] if x not in ("--renamed", "--step-keys")]
a, b = kernels(args[0]), kernels(args[1])
ka = {n for n in a if n + ".kd" in a}
kb = {n for n in b if n + ".kd" in b}
print("kernels: before %d, after %d; k_step: %d / %d" % (len(ka), len(kb), sum("k_step" in n for n in ka), sum("k_step" in n for n in kb)))
print("only in the first:", sorted(ka - kb)[:5], "only in the second:", sorted(kb - ka)[:5])
diff = [n for n in sorted(ka & kb) if a[n] != b[n] or a[n + ".kd"] != b[n + ".kd"]]
print("names compared: %d, differences: %d" % (len(ka & kb), len(diff)), diff[:5])
other = sorted(n for n in set(a) ^ set(b))
print("other symbols in one object only:", other[:10])
if renamed:
    new = {(b[n][1], b[n + ".kd"][2]) for n in kb - ka}
    lost = sorted(n for n in ka - kb if (a[n][1], a[n + ".kd"][2]) not in new)
    print("renamed: %d kernels of the first object only, %d of the second only; of the first, without a twin in code and descriptor: %d"
          % (len(ka - kb), len(kb - ka), len(lost)), lost[:5])
    sys.exit(1 if diff or lost else 0)
if step_keys:
    old = {n: step_key(n) for n in ka - kb}
    new = {step_key(n): n for n in kb - ka}
    unpaired = sorted(n for n, k in old.items() if k is None or k not in new) + sorted(n for k, n in new.items() if k is None or k not in old.values())
    pairs = [(n, new[k]) for n, k in sorted(old.items()) if k in new and k is not None]
    differ = [(n, m) for n, m in pairs if a[n] != b[m] or a[n + ".kd"] != b[m + ".kd"]]
    print("step keys: %d pairs k_step<fifteen arguments> / k_step<key>, differences in code or descriptor: %d, unpaired: %d"
          % (len(pairs), len(differ), len(unpaired)), differ[:3], unpaired[:5])
    sys.exit(1 if diff or differ or unpaired or len(old) != len(new) else 0)
sys.exit(1 if diff or ka != kb else 0)
