#!/usr/bin/env python3
"""sha256 of the device .text section of every kernel object of two builds of this repository
(the gfx950 code object unbundled from each object's .hip_fatbin section), side by side: what a
change that must be purely additive on the device side commits as its record
(profiles/*/device_code_identity.txt).

    python tools/device_code_identity.py PARENT_BUILD_DIR THIS_BUILD_DIR [--arch gfx950] > identity.txt

The build directories are the ``build/native`` of the two trees (``*.hip.o``). Uses the ROCm LLVM
tools (llvm-objcopy, clang-offload-bundler) under $ROCM_PATH.
"""
import glob
import hashlib
import os
import subprocess
import sys
import tempfile

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
BIN = os.path.join(ROCM, "llvm", "bin")


def text_of(obj, arch, tmp):
    fat, co, txt = (os.path.join(tmp, n) for n in ("fat.bin", "code.o", "text.bin"))
    subprocess.run([os.path.join(BIN, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", obj, fat], check=True)
    subprocess.run([os.path.join(BIN, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={fat}",
                    f"--targets=hipv4-amdgcn-amd-amdhsa--{arch}", f"--output={co}"], check=True, capture_output=True)
    subprocess.run([os.path.join(BIN, "llvm-objcopy"), "-O", "binary", "--only-section=.text", co, txt], check=True)
    with open(txt, "rb") as f:
        return f.read()


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    arch = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--arch=")), "gfx950")
    if len(args) != 2:
        sys.exit(__doc__)
    parent, this = args
    names = sorted({os.path.basename(p) for d in (parent, this) for p in glob.glob(os.path.join(d, "*.hip.o"))})
    print("sha256 of the device .text section (gfx950 code object unbundled from the .hip_fatbin section) of every "
          "kernel object, parent commit's build against this tree's build")
    same = diff = 0
    new = []
    with tempfile.TemporaryDirectory() as tmp:
        for n in names:
            a, b = os.path.join(parent, n), os.path.join(this, n)
            src = n[:-2]
            if not os.path.exists(a):
                new.append(src)
                continue
            if not os.path.exists(b):
                print(f"{src:28s} missing from this build")
                diff += 1
                continue
            ta, tb = text_of(a, arch, tmp), text_of(b, arch, tmp)
            ha, hb = hashlib.sha256(ta).hexdigest()[:16], hashlib.sha256(tb).hexdigest()[:16]
            ok = ta == tb
            same, diff = same + ok, diff + (not ok)
            print(f"{src:28s} {len(tb):9d} bytes  parent {ha}  this {hb}  {'same' if ok else 'DIFFERENT'}")
    extra = f" ({', '.join(new)} {'is' if len(new) == 1 else 'are'} new and {'has' if len(new) == 1 else 'have'} no counterpart)" if new else ""
    print(f"{same} identical, {diff} different{extra}")
    sys.exit(1 if diff else 0)


if __name__ == "__main__":
    main()
