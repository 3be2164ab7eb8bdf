"""Build the diagnostic (-DDS_STAMPS) library with a phase stamp after every __syncthreads() of the listed kernels.

    python tools/stamp_build.py k_edge_geom:8 k_edge_update:16 k_node_update:24
    DIFFSPECTRA_HIP_LIB=diffspectra_amd/libdiffspectra_hip_stamps.so python tools/time_forward.py ...
Counter index base follows the colon; shares print as P<base+i>.  Development tool, never part of the product build.
"""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402


def stamp_kernel(s, name, base):
    a = s.index("void %s(Ctx c" % name)
    a = s.index("{\n", a)
    b = s.index("\n}\n", a)
    k = s[a:b]
    parts = k.split("  __syncthreads();\n")
    out = parts[0]
    if "DS_STAMP_INIT" not in out:
        out = out[:2] + "  DS_STAMP_INIT();\n" + out[2:]
    for i, pt in enumerate(parts[1:]):
        out += "  __syncthreads();\n  DS_STAMP(%d);\n" % (base + i) + pt
    out += "\n  DS_STAMP(%d);\n  DS_STAMP_FLUSH(0);" % (base + len(parts) - 1)
    return s[:a] + out + s[b:], len(parts)


def strip_stamps(s):
    """Drop the in-tree stamps: they are re-inserted uniformly."""
    s = re.sub(r"\n\s*DS_STAMP(_W)?\(\d+\);", "", s)
    s = re.sub(r"\n\s*DS_STAMP_FLUSH\([^)]*\);", "", s)
    return s.replace("  DS_STAMP_INIT();\n", "")


def main():
    texts = {}                                  # source path -> stamped text, for the sources that hold a named kernel
    for spec in sys.argv[1:]:
        name, base = spec.split(":")
        holds = [p for p in g.HIP_SOURCES if "void %s(Ctx c" % name in (texts.get(p) or open(p).read())]
        if len(holds) != 1:
            sys.exit("%s: found in %d sources" % (name, len(holds)))
        src = holds[0]
        texts[src], n = stamp_kernel(texts.get(src) or strip_stamps(open(src).read()), name, int(base))
        print(name, "(%s)" % os.path.basename(src), "phases:", n, "-> P%d..P%d" % (int(base), int(base) + n - 1))
    objs = [os.path.join(g.OBJ_DIR, os.path.basename(p)[:-4] + ".o") for p in g.HIP_SOURCES]      # run build() first
    made = []
    try:
        for src, text in texts.items():
            tmp, obj = src[:-4] + "_stamped.hip", os.path.join(g.OBJ_DIR, os.path.basename(src)[:-4] + "_stamped.o")
            made += [tmp, obj]
            with open(tmp, "w") as f:
                f.write(text)
            subprocess.run(["/opt/rocm/bin/hipcc", *g.BASE_FLAGS, *g.OPT_FLAGS, "-DDS_STAMPS", "-c", tmp, "-o", obj], check=True, cwd=ROOT)
            objs[g.HIP_SOURCES.index(src)] = obj
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-shared", "-fPIC", *objs, "-o",
                        os.path.join(ROOT, "diffspectra_amd", "libdiffspectra_hip_stamps.so")], check=True)
    finally:
        for f in made:
            if os.path.exists(f):
                os.remove(f)


if __name__ == "__main__":
    main()
