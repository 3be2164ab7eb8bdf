"""Compare the gfx950 device code of two builds, kernel by kernel: `python tools/compare_device_code.py OLD_OBJ_DIR NEW_OBJ_DIR`.

The gfx950 code object of every object in either directory is unbundled and disassembled; for every kernel the instruction stream and
the metadata that decides occupancy (VGPR / SGPR / AGPR counts, LDS and scratch sizes, workgroup size limit) must be identical; only the
pc-relative distance from a kernel to a constant table in .rodata is left out, since it changes whenever kernels are emitted in another order,
and the "..." that the disassembler prints for the zero padding behind a kernel, which depends on what follows it in .text.  Kernels are
matched by their base name plus template arguments as the demangler prints them, over all objects of a directory: a kernel may move to another
object, and every report says which object it was found in on each side; a name that exists on one side only is reported as a
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
        elif cur and line.strip() and line.strip() != "...":
            insn = re.sub(r"\s*//.*$", "", line.strip())                  # the trailing comment holds the address
            if code[cur] and code[cur][-1].startswith("s_getpc_b64") and insn.startswith("s_add_u32"):
                insn = re.sub(r"0x[0-9a-f]+$", "<pc-relative>", insn)    # distance to a constant table: moves with the order of the kernels in .text
            code[cur].append(insn)
    names = run("c++filt", *meta).splitlines()
    # anonymous-namespace kernels: keep "k_name<args>" - a kernel that stops being a template keeps its base name
    short = [re.sub(r"\(.*$", "", re.sub(r"^(?:void )?(?:\(anonymous namespace\)::|\w+::)*", "", n)) for n in names]
    return {s: (code[m], meta[m]) for s, m in zip(short, meta)}


def build_kernels(obj_dir, tmp):
    """{kernel name: (object, instructions, metadata)} over every object of a build directory."""
    found = {}
    for obj in sorted(f for f in os.listdir(obj_dir) if f.endswith(".o")):
        for name, (code, meta) in kernels(os.path.join(obj_dir, obj), tmp).items():
            name = re.sub(r"<.*$", "", name) if name.startswith("k_equi_pairs") else name
            if name in found:
                raise SystemExit(f"{obj_dir}: {name} is in {found[name][0]} and in {obj}")
            found[name] = (obj, code, meta)
    return found


def main(old_dir, new_dir):
    total = differ = 0
    with tempfile.TemporaryDirectory() as t_old, tempfile.TemporaryDirectory() as t_new:
        old, new = build_kernels(old_dir, t_old), build_kernels(new_dir, t_new)
    for name in sorted(set(old) | set(new)):
        total += 1
        if name not in old or name not in new:
            differ += 1
            print(f"{name}: only in the {'new' if name in new else 'old'} build ({(new if name in new else old)[name][0]})")
            continue
        (o_obj, o_code, o_meta), (n_obj, n_code, n_meta) = old[name], new[name]
        where = o_obj if o_obj == n_obj else f"{o_obj} -> {n_obj}"
        if (o_code, o_meta) != (n_code, n_meta):
            differ += 1
            what = "metadata" if o_meta != n_meta else "instructions"
            print(f"{where}: {name}: {what} differ ({len(o_code)} vs {len(n_code)} instructions; {o_meta} vs {n_meta})")
        elif o_obj != n_obj:
            print(f"{where}: {name}: identical")
    print(f"{total} kernels compared, {differ} differ")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
