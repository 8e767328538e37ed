#!/usr/bin/env python3
"""Device-code identity of a refactor: a git revision against the working tree, gfx950, compile only (no GPU needed).

    python tools/code_identity.py [--rev HEAD~1] [--jobs 8] [--work DIR] ppo_policy_bwd ppo_policy_fwd ...

Per named csrc/*.hip: hipcc with the Makefile's FLAGS plus --offload-device-only -c on both sides (the older side is
`git show REV:path` of the file and of that revision's headers, in a temporary directory laid out like the tree);
the gfx950 code object is unbundled where hipcc bundles it; llvm-objcopy -O binary --only-section=.text gives the bytes
that are hashed; llvm-readelf --notes gives the AMDGPU metadata, compared kernel by kernel (VGPRs, SGPRs, scratch, LDS,
kernarg layout) and by the number of kernels.  Prints one block per file and exits non-zero on any difference.
--work DIR keeps the objects there, and reuses the older side's where DIR already holds them for the same commit."""
import argparse
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "proximalpolicyoptimization.jl_amd"
CSRC = os.path.join(PKG, "csrc")
MAX_JOBS = 16


def llvm_bin():
    hipcc = shutil.which(os.environ.get("HIPCC", "hipcc"))
    roots = [os.environ.get("ROCM_PATH"), os.path.dirname(os.path.dirname(os.path.realpath(hipcc))) if hipcc else None, "/opt/rocm"]
    for r in filter(None, roots):
        for sub in ("lib/llvm/bin", "llvm/bin"):
            if os.path.exists(os.path.join(r, sub, "llvm-objcopy")):
                return os.path.join(r, sub)
    sys.exit("code_identity: no llvm-objcopy / llvm-readelf / clang-offload-bundler under a ROCm root")


def makefile_flags(arch):
    text = open(os.path.join(ROOT, CSRC, "Makefile")).read()
    flags = re.search(r"^FLAGS\s*=\s*(.*)$", text, re.M).group(1)
    return flags.replace("$(ARCH)", arch).split()


def git(*args):
    return subprocess.run(["git", "-C", ROOT] + list(args), check=True, capture_output=True).stdout


def export_rev(rev, dst, names):
    """REV's headers (csrc/*.h, include/*.h) and the named sources, under dst in the tree's own layout"""
    listed = git("ls-tree", "-r", "--name-only", rev, "--", CSRC, "include").decode().split()
    for path in listed:
        if path.endswith(".h") or (path.endswith(".hip") and os.path.basename(path)[:-4] in names):
            out = os.path.join(dst, path)
            os.makedirs(os.path.dirname(out), exist_ok=True)
            with open(out, "wb") as f:
                f.write(git("show", "%s:%s" % (rev, path)))


def device_object(tools, flags, csrc_dir, name, out):
    """compile csrc_dir/name.hip for the device only; out = the gfx950 ELF"""
    raw = out + ".raw"
    subprocess.run([os.environ.get("HIPCC", "hipcc")] + flags + ["--offload-device-only", "-c", name + ".hip", "-o", raw],
                   cwd=csrc_dir, check=True)
    with open(raw, "rb") as f:
        magic = f.read(24)
    if magic.startswith(b"\x7fELF"):
        os.replace(raw, out)
        return
    listed = subprocess.run([os.path.join(tools, "clang-offload-bundler"), "--list", "--type=o", "--input=" + raw],
                            check=True, capture_output=True, text=True).stdout.split()
    target = [t for t in listed if "amdgcn" in t]
    assert len(target) == 1, "expected one device entry in the bundle, found %r" % listed
    subprocess.run([os.path.join(tools, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=" + target[0],
                    "--input=" + raw, "--output=" + out], check=True)
    os.remove(raw)


def section_sizes(tools, obj):
    out = subprocess.run([os.path.join(tools, "llvm-readelf"), "-S", "-W", obj], check=True, capture_output=True, text=True).stdout
    sizes = {}
    for m in re.finditer(r"\]\s+(\.\S+)\s+\S+\s+[0-9a-f]+\s+[0-9a-f]+\s+([0-9a-f]+)", out):
        sizes[m.group(1)] = int(m.group(2), 16)
    return sizes


def text_bytes(tools, obj):
    binf = obj + ".text"
    subprocess.run([os.path.join(tools, "llvm-objcopy"), "-O", "binary", "--only-section=.text", obj, binf], check=True)
    with open(binf, "rb") as f:
        return f.read()


def kernel_notes(tools, obj):
    """{kernel name: its entry of amdhsa.kernels as text}, plus what the note holds besides the kernels"""
    out = subprocess.run([os.path.join(tools, "llvm-readelf"), "--notes", obj], check=True, capture_output=True, text=True).stdout
    kernels, rest, cur, inside = {}, [], None, False
    for line in out.splitlines():
        if line.startswith("amdhsa.kernels:"):
            inside = True
        elif inside and line.startswith("  - "):
            cur = [line]
            kernels[len(kernels)] = cur
        elif inside and (line.startswith("    ") or not line.strip()) and cur is not None:
            cur.append(line)
        else:
            inside, cur = False, None
            if not re.search(r"NT_AMDGPU_METADATA|Owner\s+Data size|Displaying notes", line):    # the note's own byte count
                rest.append(line)
    named = {}
    for block in kernels.values():
        body = "\n".join(block)
        named[re.search(r"^\s+\.name:\s+(\S+)", body, re.M).group(1)] = body
    assert len(named) == len(kernels), "two kernels of one name"
    return named, "\n".join(rest)


def examine(tools, obj):
    text = text_bytes(tools, obj)
    sizes = section_sizes(tools, obj)
    kernels, rest = kernel_notes(tools, obj)
    return {"text": text, "sha": hashlib.sha256(text).hexdigest(), "sizes": sizes, "kernels": kernels, "rest": rest}


def report(name, rev_label, old, new):
    lines = [name + ".hip"]
    for label, side in ((rev_label, old), ("tree", new)):
        lines.append("  %-6s .text %8d bytes  sha256 %s  (.rodata %d bytes, .dynstr %d bytes)" % (
            label, len(side["text"]), side["sha"], side["sizes"].get(".rodata", 0), side["sizes"].get(".dynstr", 0)))
    same_text = old["text"] == new["text"]
    differing = sorted(k for k in set(old["kernels"]) | set(new["kernels"]) if old["kernels"].get(k) != new["kernels"].get(k))
    same_meta = not differing and old["rest"] == new["rest"] and len(old["kernels"]) == len(new["kernels"])
    lines.append("  .text byte-identical: %s; metadata notes identical: %s (%d kernels%s)" % (
        "yes" if same_text else "NO", "yes" if same_meta else "NO", len(new["kernels"]),
        "" if len(old["kernels"]) == len(new["kernels"]) else ", %s has %d" % (rev_label, len(old["kernels"]))))
    if not same_text and len(old["text"]) == len(new["text"]):
        first = next(i for i, (a, b) in enumerate(zip(old["text"], new["text"])) if a != b)
        lines.append("    same size; first differing byte at .text + 0x%x" % first)
    for k in differing[:8]:
        lines.append("    metadata differs: %s" % k)
        a, b = (side["kernels"].get(k, "").splitlines() for side in (old, new))
        for la, lb in zip(a, b):
            if la != lb:
                lines.append("      %s  ->  %s" % (la.strip(), lb.strip()))
        if len(a) != len(b):
            lines.append("      %d -> %d lines" % (len(a), len(b)))
    return same_text and same_meta, "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("files", nargs="+", help="csrc sources, with or without .hip")
    ap.add_argument("--rev", default="HEAD~1")
    ap.add_argument("--arch", default="gfx950")
    ap.add_argument("--jobs", type=int, default=min(MAX_JOBS, os.cpu_count() or 1))
    ap.add_argument("--work", help="keep the objects here; reuse the revision's objects found here")
    a = ap.parse_args()
    names = [os.path.basename(f)[:-4] if f.endswith(".hip") else os.path.basename(f) for f in a.files]
    tools, flags = llvm_bin(), makefile_flags(a.arch)
    sha = git("rev-parse", a.rev).decode().strip()
    work = a.work or tempfile.mkdtemp(prefix="ppo_code_identity_")
    old_root, new_out = os.path.join(work, sha[:12]), os.path.join(work, "tree")
    os.makedirs(new_out, exist_ok=True)
    export_rev(sha, old_root, names)

    def side(which, name):
        if which == "old":
            out = os.path.join(old_root, name + ".co")
            if not os.path.exists(out):
                device_object(tools, flags, os.path.join(old_root, CSRC), name, out)
        else:
            out = os.path.join(new_out, name + ".co")
            device_object(tools, flags, os.path.join(ROOT, CSRC), name, out)
        return examine(tools, out)

    try:
        with ThreadPoolExecutor(max(1, min(a.jobs, MAX_JOBS))) as pool:
            jobs = {(w, n): pool.submit(side, w, n) for n in names for w in ("tree", "old")}
            ok = True
            for n in names:
                same, text = report(n, a.rev, jobs[("old", n)].result(), jobs[("tree", n)].result())
                ok &= same
                print(text, flush=True)
    finally:
        if not a.work:
            shutil.rmtree(work, ignore_errors=True)
    print("device code identical to %s (%s): %s" % (a.rev, sha[:12], "yes" if ok else "NO"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
