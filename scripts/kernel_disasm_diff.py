"""Compare the gfx950 disassembly of every kernel symbol between two builds of flash_attention_dlrs_amd/csrc.

    python scripts/kernel_disasm_diff.py OLD_CSRC_DIR NEW_CSRC_DIR

Each directory holds the objects `make` left there (fa2_*.o).  The device code object of every object file is unbundled
(clang-offload-bundler), disassembled (llvm-objdump -d) and split per function symbol.  Every symbol of the old build must
exist in the new one with the same instructions; symbols only in the new build are listed.  Exit status 1 on a difference.
"""
import glob
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def symbols(obj, tmp):
    fat = os.path.join(tmp, "fatbin")
    dev = os.path.join(tmp, "dev.co")
    if subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", obj, os.path.join(tmp, "host.o")],
                      capture_output=True).returncode != 0:
        return {}
    subprocess.check_call([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}",
                           f"--targets={TARGET}", f"--output={dev}"])
    text = subprocess.check_output([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", dev], text=True)
    out, name, body = {}, None, []
    for line in text.splitlines():
        m = re.match(r"^(?:[0-9a-f]+ )?<(.+)>:$", line)
        if m:
            if name:
                out[name] = body
            name, body = m.group(1), []
        elif name and line.strip():
            body.append(re.sub(r"\s*//.*$", "", line).strip())  # drop the address / encoding comments
    if name:
        out[name] = body
    return out


def collect(d):
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        for obj in sorted(glob.glob(os.path.join(d, "fa2_*.o"))):
            if obj.endswith(("_asan.o", "_abl.o", "_exp.o", "_st.o", "_var.o", "_blob.o")):
                continue
            for k, v in symbols(obj, tmp).items():
                res[k] = v
    return res


def main():
    old, new = collect(sys.argv[1]), collect(sys.argv[2])
    changed = [k for k in old if k not in new or new[k] != old[k]]
    added = sorted(k for k in new if k not in old)
    print(f"{len(old)} kernel symbols in the old build, {len(old) - len(changed)} identical, {len(changed)} changed or missing")
    for k in changed:
        print("  CHANGED" if k in new else "  MISSING", k)
    print(f"{len(added)} new symbols")
    for k in added:
        print("  NEW", k)
    return 1 if changed else 0


if __name__ == "__main__":
    sys.exit(main())
