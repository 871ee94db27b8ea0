#!/usr/bin/env python3
"""Is the device code of this tree the same as that of another commit, kernel by kernel?

A refactor of the HIP sources must not change code generation: the kernels are the speed of the library.  This compiles every
translation unit of orb_slam3-1_amd/csrc (what its Makefile builds) of a base commit and of the working tree to gfx950
assembly, device side only, with the Makefile's flags, cuts each listing at its kernels, and compares the instruction streams and
the kernel descriptors (registers, LDS, scratch).  Kernels are matched by their unqualified name and parameter list, so moving one
into another namespace or file of the same unit does not count; comments are dropped and the numbers of local labels
(.LBB<k>_<i>, .Ltmp<k>), which change whenever functions are reordered, are normalised.  Needs no GPU.

    python tools/kernel_asm_diff.py                 # working tree against HEAD
    python tools/kernel_asm_diff.py --base main~3
    python tools/kernel_asm_diff.py --base-dir /some/checkout/orb_slam3-1_amd/csrc
    python tools/kernel_asm_diff.py --renamed 'k_errors_kb8=k_errors<kb8::Cam>'     # a base kernel that has another name here

--renamed OLD=NEW (repeatable) names the function without its namespaces and parameters, with its template arguments: the base
kernel OLD is compared with the kernel NEW of the working tree.  Lines that only switch the section (.text, or the comdat section
.text.<name> a template instantiation is emitted into) are neither instructions nor descriptors and are dropped.

Exit status 0: same set of kernels, all identical.  1: a kernel differs, is missing or is new (each is listed; --show prints a
unified diff of the first lines that differ).
"""
import argparse
import concurrent.futures
import difflib
import os
import re
import subprocess
import sys
import tarfile
import tempfile
import io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "orb_slam3-1_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CXXFILT = os.environ.get("CXXFILT", "c++filt")
FLAGS = ["-O3", "--offload-arch=gfx950", "-ffp-contract=off", "-fPIC", "-std=c++17", "--cuda-device-only", "-S"]


def units(csrc):
    """the .hip files the Makefile builds (orbx_kernels.hip is included by orbx_extractor.hip)"""
    return sorted(f for f in os.listdir(csrc) if f.endswith(".hip") and f != "orbx_kernels.hip")


def compile_unit(csrc, unit, out_dir, defines):
    out = os.path.join(out_dir, unit[:-4] + ".s")
    subprocess.run([HIPCC] + FLAGS + ["-D" + d for d in defines] + ["-o", out, unit], cwd=csrc, check=True, stderr=subprocess.PIPE)
    return out


def demangle(names):
    if not names:
        return {}
    res = subprocess.run([CXXFILT], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    return dict(zip(names, res))


def unqualified(demangled):
    """'void lba::k_x<true>(lba::Dev, int)' -> 'k_x<true>(lba::Dev, int)': the function's own namespaces go, its parameters stay"""
    m = re.match(r"^(?:void )?((?:\w+::)*)(\w+(?:<.*?>)?)(\(.*\))$", demangled)
    if not m:
        return demangled
    return m.group(2) + re.sub(r"(\(|, ), ", r"\1", m.group(3))       # (c++filt leaves an empty slot, "(A, , B)", where a parameter pack is empty)


def kernel_symbols(lines):
    return [m.group(1) for ln in lines for m in [re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)] if m]


def kernels_of(listing):
    """{key: [normalised lines]} of one assembly listing"""
    lines = open(listing).read().splitlines()
    return kernels_of_lines(lines, {n: unqualified(d) for n, d in demangle(kernel_symbols(lines)).items()}, listing)


def kernels_of_lines(lines, pretty, listing="listing"):
    """the same of a listing's lines; pretty = {kernel symbol: its key, the unqualified demangled name}"""
    names = kernel_symbols(lines)
    start = {}
    for i, ln in enumerate(lines):
        m = re.match(r"^([A-Za-z_$][\w$.]*):", ln)
        if m and m.group(1) in pretty:
            start[m.group(1)] = i
    out = {}
    for n in names:
        body = []
        i = start[n] + 1
        while not re.match(r"^\.Lfunc_end\d+:", lines[i]):
            body.append(lines[i])
            i += 1
        j = next(k for k, ln in enumerate(lines) if re.match(r"\s*\.amdhsa_kernel\s+" + re.escape(n) + r"\s*$", ln))
        while not re.match(r"\s*\.end_amdhsa_kernel", lines[j]):
            body.append(lines[j])
            j += 1
        if pretty[n] in out:        # two namespaces of one unit with the same kernel signature: one would go uncompared
            raise SystemExit("%s: two kernels are both '%s' once their namespaces are dropped; rename one" % (listing, pretty[n]))
        out[pretty[n]] = normalise(body, pretty)
    return out


def normalise(body, pretty):
    res, tmp = [], {}
    for ln in body:
        ln = ln.split(";", 1)[0].strip()            # comments
        if not ln or re.match(r"^(\.text|\.section\s+\.text\.\S*,comdat)$", ln):     # ... and switches of the section
            continue
        ln = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", ln)
        ln = re.sub(r"\.Ltmp\d+", lambda m: tmp.setdefault(m.group(0), ".Ltmp_%d" % len(tmp)), ln)
        ln = re.sub(r"_Z[\w$.]+", lambda m: pretty.get(m.group(0), m.group(0)), ln)     # a kernel's own (mangled) name
        res.append(re.sub(r"\s+", " ", ln))
    return res


def rename_base(kb, renames):
    """the base kernels of one unit under their names here: [(old, new)] on the name in front of the parameter list"""
    out = {}
    for key, body in kb.items():
        for old, new in renames:
            if key.startswith(old + "("):
                new_key = new + key[len(old):]
                key, body = new_key, [ln.replace(key, new_key) for ln in body]
                break
        out[key] = body
    return out


def compare(kb, kh, renames=()):
    """(identical, differ, missing, new) keys of one unit, base against here"""
    kb = rename_base(kb, renames)
    same = [k for k in kb if k in kh and kb[k] == kh[k]]
    differ = [k for k in kb if k in kh and kb[k] != kh[k]]
    return same, differ, [k for k in kb if k not in kh], [k for k in kh if k not in kb]


def listing_set(csrc, out_dir, defines, jobs):
    us = units(csrc)
    with concurrent.futures.ThreadPoolExecutor(jobs) as ex:
        files = list(ex.map(lambda u: compile_unit(csrc, u, out_dir, defines), us))
    return {u: kernels_of(f) for u, f in zip(us, files)}


def export_base(rev, to):
    tar = subprocess.run(["git", "-C", ROOT, "archive", rev, "orb_slam3-1_amd/csrc", "include"], check=True, capture_output=True).stdout
    tarfile.open(fileobj=io.BytesIO(tar)).extractall(to)
    return os.path.join(to, "orb_slam3-1_amd", "csrc")


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--base", default="HEAD", help="commit to compare the working tree against")
    ap.add_argument("--base-dir", help="a csrc directory to compare against instead of a commit")
    ap.add_argument("-D", dest="defines", action="append", default=[], help="extra macro for both sides (e.g. LBA_STEP_TIMING)")
    ap.add_argument("-j", dest="jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--renamed", action="append", default=[], metavar="OLD=NEW", help="a base kernel OLD is the kernel NEW here (repeatable)")
    ap.add_argument("--show", action="store_true", help="print a diff of every kernel that differs")
    args = ap.parse_args()
    renames = [tuple(r.split("=", 1)) for r in args.renamed]
    with tempfile.TemporaryDirectory() as tmp:
        base_csrc = args.base_dir or export_base(args.base, os.path.join(tmp, "base"))
        os.makedirs(os.path.join(tmp, "a")), os.makedirs(os.path.join(tmp, "b"))
        base = listing_set(base_csrc, os.path.join(tmp, "a"), args.defines, args.jobs)
        here = listing_set(CSRC, os.path.join(tmp, "b"), args.defines, args.jobs)
    bad = 0
    for u in sorted(set(base) | set(here)):
        kb, kh = rename_base(base.get(u, {}), renames), here.get(u, {})
        same, differ, gone, new = compare(kb, kh)
        print("%-22s %3d kernels in the base, %3d here: %3d identical, %d differ, %d missing, %d new" % (u, len(kb), len(kh), len(same), len(differ), len(gone), len(new)))
        for tag, ks in (("differs", differ), ("missing", gone), ("new", new)):
            for k in ks:
                print("    %s: %s" % (tag, k))
        if args.show:
            for k in differ:
                print("\n".join(list(difflib.unified_diff(kb[k], kh[k], "base " + k, "here " + k, lineterm="", n=2))[:60]))
        bad += len(differ) + len(gone) + len(new)
    print("device code identical" if not bad else "%d kernels differ" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
