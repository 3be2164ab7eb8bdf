"""Compare the gfx950 device code of two builds, kernel by kernel: `python tools/compare_device_code.py OLD_OBJ_DIR NEW_OBJ_DIR`.

For every object present in both directories the gfx950 code object is unbundled and disassembled; for every kernel the instruction stream and
the metadata that decides occupancy (VGPR / SGPR / AGPR counts, LDS and scratch sizes, workgroup size limit) must be identical; only the
pc-relative distance from a kernel to a constant table in .rodata is left out, since it changes whenever kernels are emitted in another order.  Kernels are
matched by their base name plus template arguments as the demangler prints them; a name that exists on one side only is reported as a
difference.  Prints "N kernels compared, M differ" and exits non-zero when M > 0: what a refactor of the host code has to show."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM_BIN", "/opt/rocm/llvm/bin")
META = (".vgpr_count", ".sgpr_count", ".agpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size", ".max_flat_workgroup_size",
        ".vgpr_spill_count", ".sgpr_spill_count", ".kernarg_segment_size")


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def kernels(obj, tmp):
    """{demangled kernel name: (instructions, metadata)} of the gfx950 code object bundled in a host object."""
    fat, co = os.path.join(tmp, os.path.basename(obj) + ".fatbin"), os.path.join(tmp, os.path.basename(obj) + ".co")
    run(os.path.join(LLVM, "llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", obj, os.path.join(tmp, "copy.o"))
    run(os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fat}", f"--output={co}")
    meta = {}
    for block in run(os.path.join(LLVM, "llvm-readelf"), "--notes", co).split("  - .agpr_count")[1:]:
        block = ".agpr_count" + block
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = {k: re.search(re.escape(k) + r":\s+(\S+)", block).group(1) for k in META if k + ":" in block}
    code, cur = {}, None
    for line in run(os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co).splitlines():
        m = re.match(r"^<(\w+)>:$", line.strip()) if line and not line.startswith((" ", "\t")) else None
        if m:
            cur = m.group(1)
            code[cur] = []
        elif cur and line.strip():
            insn = re.sub(r"\s*//.*$", "", line.strip())                  # the trailing comment holds the address
            if code[cur] and code[cur][-1].startswith("s_getpc_b64") and insn.startswith("s_add_u32"):
                insn = re.sub(r"0x[0-9a-f]+$", "<pc-relative>", insn)    # distance to a constant table: moves with the order of the kernels in .text
            code[cur].append(insn)
    names = run("c++filt", *meta).splitlines()
    # anonymous-namespace kernels: keep "k_name<args>" - a kernel that stops being a template keeps its base name
    short = [re.sub(r"\(.*$", "", re.sub(r"^(?:void )?(?:\(anonymous namespace\)::|\w+::)*", "", n)) for n in names]
    return {s: (code[m], meta[m]) for s, m in zip(short, meta)}


def main(old_dir, new_dir):
    total = differ = 0
    with tempfile.TemporaryDirectory() as t_old, tempfile.TemporaryDirectory() as t_new:
        for obj in sorted(f for f in os.listdir(old_dir) if f.endswith(".o") and os.path.exists(os.path.join(new_dir, f))):
            old, new = kernels(os.path.join(old_dir, obj), t_old), kernels(os.path.join(new_dir, obj), t_new)
            base = lambda d: {re.sub(r"<.*$", "", k) if k.startswith("k_equi_pairs") else k: v for k, v in d.items()}
            old, new = base(old), base(new)
            for name in sorted(set(old) | set(new)):
                total += 1
                if name not in old or name not in new:
                    differ += 1
                    print(f"{obj}: {name}: only in the {'new' if name in new else 'old'} build")
                elif old[name] != new[name]:
                    differ += 1
                    what = "metadata" if old[name][1] != new[name][1] else "instructions"
                    print(f"{obj}: {name}: {what} differ ({len(old[name][0])} vs {len(new[name][0])} instructions; {old[name][1]} vs {new[name][1]})")
    print(f"{total} kernels compared, {differ} differ")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
