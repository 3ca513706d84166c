#!/usr/bin/env python3
"""Is the device code of this tree the device code of another commit?  (What a host-side refactor has to show.)

For every file of pcgol_amd.build.SOURCES the device side is compiled to assembly (the flags of pcgol_amd/build.py plus
--cuda-device-only -S) from the working tree and from `git archive REV`, and compared function by function: as maps
name -> text of the functions (a kernel with its descriptor and resource comments) and of the entries of the
code-object metadata, because the order in which template instantiations are emitted follows the host's launch sites
and may move.  What moves with that order is normalised away: the function index in local labels (.LBB<i>_<n>,
.Lfunc_end<i>, the comments' BB<i>_<n>), the padding behind whichever function is emitted last, and the
__hip_cuid_<hash> symbol, which differs between two compiles of one source.

    python tools/compare_device_code.py [--rev HEAD] [--jobs 8] [--rename OLD=NEW ...] [file.hip ...]

A function that differs is listed with its instruction lines, REV's -> the tree's.  --rename: a kernel whose name
changed between the two (substrings of the mangled names) is compared with its predecessor instead of being listed
twice, once as missing and once as new.
Needs hipcc, no GPU.  Exit status 0: every function of every file is textually identical."""
import argparse
import concurrent.futures
import io
import os
import re
import subprocess
import sys
import tarfile
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pcgol_amd import build as B  # noqa: E402

BEGIN = re.compile(r"-- Begin function (\S+)")
LABEL = re.compile(r"\b(L?BB|Lfunc_end|Lfunc_begin|Ltmp)\d+")  # (BB<i>_<n> without .L: the comments' loop headers)


def device_asm(tree, src):
    cmd = [B.hipcc()] + B.flags() + ["--cuda-device-only", "-S", "-w", "-o", "-",
                                     os.path.join(tree, "pcgol_amd", "csrc", src)]
    return subprocess.run(cmd, check=True, stdout=subprocess.PIPE, cwd=tree).stdout.decode()


def split(asm):
    """-> {key: text}: 'fn NAME' per function, 'meta NAME' per metadata entry, 'rest' for what belongs to no function"""
    lines = [LABEL.sub(lambda m: m.group(1), ln) for ln in asm.splitlines() if "__hip_cuid_" not in ln]
    out, key = {"rest": []}, "rest"
    for ln in lines:
        m = BEGIN.search(ln)
        if m:
            prev = out[key]
            key = "fn " + m.group(1)
            assert key not in out, key
            # (the section switch in front of a function is the function's, not its predecessor's)
            out[key] = [prev.pop()] if prev and prev[-1].split()[:1] in ([".text"], [".section"]) else []
        elif ".AMDGPU.gpr_maximums" in ln or ln.strip() == ".amdgpu_metadata":
            key = "rest"
        elif ln.split()[:1] == [".p2alignl"]:
            # (the padding behind the code object's last function -- .text, .p2alignl, .fill -- is whichever function's
            # comes last in the emission order, not that function's)
            prev = out[key]
            key = "rest"
            out[key] += [prev.pop()] if prev and prev[-1].split()[:1] == [".text"] else []
        out[key].append(ln)
    # the metadata's kernel entries: a YAML list under amdhsa.kernels, each entry with its .name
    rest, meta, entry = [], {}, None

    def flush(entry):
        name = [x.split(":", 1)[1].strip() for x in entry or [] if x.strip().startswith(".name:") and x.startswith("    .")]
        if name:
            meta["meta " + name[0]] = entry
        else:
            rest.extend(entry or [])

    for ln in out["rest"] + [""]:
        if ln.startswith("  - ") or not ln.startswith("    "):
            flush(entry)
            entry = [] if ln.startswith("  - ") else None
        (rest if entry is None else entry).append(ln)
    out["rest"] = rest
    out.update(meta)
    return {k: "\n".join(v) for k, v in out.items()}


def instructions(text):
    """the instruction lines of a function's text: neither directives, labels nor comments"""
    lines = (ln.strip() for ln in text.splitlines())
    return sum(1 for ln in lines if ln and ln[0] not in ".;" and not ln.split(";")[0].strip().endswith(":"))


def rename(a, b, renames):
    """A kernel of the other commit that has another name here is compared under its name here: OLD and NEW are
    substrings of the mangled names, each naming one function of its side; the other side's symbol is rewritten."""
    for old, new in renames:
        olds = [k[3:] for k in b if k.startswith("fn ") and old in k]
        news = [k[3:] for k in a if k.startswith("fn ") and new in k]
        if len(olds) != 1 or len(news) != 1:
            continue  # (another file's kernel)
        b = {k.replace(olds[0], news[0]): v.replace(olds[0], news[0]) for k, v in b.items()}
    return b


def compare(src, here, there, renames=()):
    if not os.path.exists(os.path.join(there, "pcgol_amd", "csrc", src)):  # a file the other commit does not have
        a = split(device_asm(here, src))
        return src, sum(k.startswith("fn ") for k in a), sum(k.startswith("meta ") for k in a), None
    a, b = split(device_asm(here, src)), split(device_asm(there, src))
    b = rename(a, b, renames)
    differing = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
    # (a function that differs: its instruction lines there -> here; "-" where one side does not have it)
    differing = [k + ("   instructions %s -> %s" % tuple(instructions(m[k]) if k in m else "-" for m in (b, a))
                      if k.startswith("fn ") else "") for k in differing]
    return src, sum(k.startswith("fn ") for k in a), sum(k.startswith("meta ") for k in a), differing


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rev", default="HEAD", help="the commit to compare the working tree with (default HEAD)")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW",
                    help="compare REV's function whose mangled name contains OLD with the tree's that contains NEW")
    ap.add_argument("sources", nargs="*", help="files of pcgol_amd/csrc (default: all of build.SOURCES)")
    args = ap.parse_args()
    renames = [tuple(r.split("=", 1)) for r in args.rename]
    sources = args.sources or B.SOURCES
    with tempfile.TemporaryDirectory() as there:
        tar = subprocess.run(["git", "-C", ROOT, "archive", args.rev, "pcgol_amd", "include"], check=True,
                             stdout=subprocess.PIPE).stdout
        tarfile.open(fileobj=io.BytesIO(tar)).extractall(there)
        with concurrent.futures.ThreadPoolExecutor(args.jobs) as pool:
            results = list(pool.map(lambda s: compare(s, ROOT, there, renames), sources))
    n_fn = n_kernels = n_diff = 0
    for src, fns, kernels, differing in results:
        if differing is None:  # (nothing to compare with: every existing function is in the other files)
            print("%-24s %3d functions (%3d kernels): new, not in %s" % (src, fns, kernels, args.rev))
            continue
        print("%-24s %3d functions (%3d kernels): %s" % (src, fns, kernels, "identical" if not differing else "DIFFER"))
        for k in differing:
            print("    " + k)
        n_fn, n_kernels, n_diff = n_fn + fns, n_kernels + kernels, n_diff + len(differing)
    print("%d files, %d functions, %d kernels compared with %s: %d differ"
          % (sum(r[3] is not None for r in results), n_fn, n_kernels, args.rev, n_diff))
    return 1 if n_diff else 0


if __name__ == "__main__":
    sys.exit(main())
