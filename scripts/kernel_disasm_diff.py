"""Compare the gfx950 code of every kernel symbol between two builds of flash_attention_dlrs_amd/csrc.

    python scripts/kernel_disasm_diff.py [--suffix SUFFIX] [--rename REGEX=REPL ...] [--kernarg-info] OLD_CSRC_DIR NEW_CSRC_DIR

Each directory holds the objects `make` left there (fa2_*.o).  The device code object of every object file is unbundled
(clang-offload-bundler), disassembled (llvm-objdump -d) and split per function symbol; the code-object metadata of every
kernel is read from the notes (llvm-readelf --notes): VGPR, AGPR and SGPR counts, spills, LDS bytes, scratch bytes, kernarg
size, max workgroup size.  Every symbol of the old build must exist in the same object of the new one with the same
instructions and the same metadata; symbols only in the new build are listed.  Exit status 1 on a difference.

llvm-objdump prints "..." for the zero bytes that pad the last instruction of a symbol up to the next symbol's alignment; whether
a symbol has them depends on what follows it in its object, not on its code, so these lines are left out of the comparison (a
kernel that moved to another unit would otherwise differ from itself).

--suffix names the objects to compare: "" (the default) for the library's own fa2_*.o, or one of _abl, _st, _var, _exp,
_asan for the objects of the other builds (fa2_*_abl.o, ...).

--rename REGEX=REPL (repeatable) maps an old symbol to its new unit and name: each is applied with re.sub to the old build's
keys, which read "<unit>: <mangled symbol>", before the two builds are matched.  --kernarg-info reports a changed
.kernarg_segment_size but does not count it as a difference (a kernel whose argument struct grew fields it never reads).
Example, a kernel that left its stub unit and macro-given name for a template argument of the plain kernel's file:

    --rename '^fa2_mfma16d_w: _ZN12_GLOBAL__N_129fa2_fwd_mfma16d_window_kernelI(.*)EEvNS=fa2_mfma16d:
              _ZN11fa2_mfma16d22fa2_fwd_mfma16d_kernelI\\g<1>Li1EEEvNS'        (one argument, no line break)
"""
import argparse
import glob
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
SUFFIXES = ("_asan", "_abl", "_exp", "_st", "_var")
META = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".group_segment_fixed_size",
        ".private_segment_fixed_size", ".kernarg_segment_size", ".max_flat_workgroup_size")


def disassembly(dev):
    text = subprocess.check_output([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", dev], text=True)
    out, name, body = {}, None, []
    for line in text.splitlines():
        m = re.match(r"^(?:[0-9a-f]+ )?<(.+)>:$", line)
        if m:
            if name:
                out[name] = body
            name, body = m.group(1), []
        elif name and line.strip() and line.strip() != "...":  # ("...": zero padding up to the next symbol's alignment)
            body.append(re.sub(r"\s*//.*$", "", line).strip())  # drop the address / encoding comments
    if name:
        out[name] = body
    return out


def metadata(dev):
    """{kernel name: {key: value}} from the amdhsa.kernels list of the code object's metadata note."""
    text = subprocess.check_output([f"{LLVM}/llvm-readelf", "--notes", dev], text=True)
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^  (-| ) (\.\w+):\s*(\S.*)?$", line)  # the scalar fields of one list entry, not its nested .args
        if not m:
            if not line.startswith("    "):
                cur = None  # left the amdhsa.kernels list
            continue
        if m.group(1) == "-":
            cur = {}
        if cur is None:
            continue
        cur[m.group(2)] = m.group(3)
        if m.group(2) == ".name":
            out[m.group(3)] = cur
    return {k: {f: v.get(f) for f in META} for k, v in out.items()}


def symbols(obj, tmp):
    """{symbol: (instructions, metadata or None)} of the device code in one host object."""
    fat = os.path.join(tmp, "fatbin")
    dev = os.path.join(tmp, "dev.co")
    if subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", obj, os.path.join(tmp, "host.o")],
                      capture_output=True).returncode != 0:
        return {}
    subprocess.check_call([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}",
                           f"--targets={TARGET}", f"--output={dev}"])
    meta = metadata(dev)
    return {k: (v, meta.get(k)) for k, v in disassembly(dev).items()}


def collect(d, suffix):
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        for obj in sorted(glob.glob(os.path.join(d, f"fa2_*{suffix}.o"))):
            stem = os.path.basename(obj)[:-2]
            if "_blob" in stem or (not suffix and stem.endswith(SUFFIXES)):
                continue
            unit = stem[:len(stem) - len(suffix)] if suffix else stem
            for k, v in symbols(obj, tmp).items():
                res[f"{unit}: {k}"] = v
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--suffix", default="", choices=("",) + SUFFIXES, help="object suffix to compare (default: none)")
    ap.add_argument("--rename", action="append", default=[], metavar="REGEX=REPL", help="re.sub applied to the old build's keys")
    ap.add_argument("--kernarg-info", action="store_true", help="a changed .kernarg_segment_size is reported, not counted")
    ap.add_argument("old")
    ap.add_argument("new")
    args = ap.parse_args()
    old, new = collect(args.old, args.suffix), collect(args.new, args.suffix)
    for pat, repl in (r.split("=", 1) for r in args.rename):
        old = {re.sub(pat, repl, k): v for k, v in old.items()}
    if args.kernarg_info:
        moved = [k for k in old if k in new and old[k][1] and new[k][1]
                 and old[k][1][".kernarg_segment_size"] != new[k][1][".kernarg_segment_size"]]
        print(f"{len(moved)} kernels with another .kernarg_segment_size (informational)")
        for k in moved:
            print("  KERNARG", k, old[k][1][".kernarg_segment_size"], "->", new[k][1][".kernarg_segment_size"])
            new[k] = (new[k][0], dict(new[k][1], **{".kernarg_segment_size": old[k][1][".kernarg_segment_size"]}))
    kernels = sum(1 for v in old.values() if v[1] is not None)
    changed = [k for k in old if k not in new or new[k] != old[k]]
    added = sorted(k for k in new if k not in old)
    print(f"{len(old)} symbols ({kernels} kernels with metadata) in the old build, {len(old) - len(changed)} identical, "
          f"{len(changed)} changed or missing")
    for k in changed:
        if k not in new:
            print("  MISSING", k)
            continue
        what = [w for w, i in (("instructions", 0), ("metadata", 1)) if new[k][i] != old[k][i]]
        print("  CHANGED", k, "(" + ", ".join(what) + ")")
        if "metadata" in what:
            print("    old", old[k][1])
            print("    new", new[k][1])
    print(f"{len(added)} new symbols")
    for k in added:
        print("  NEW", k)
    return 1 if changed or added else 0


if __name__ == "__main__":
    sys.exit(main())
