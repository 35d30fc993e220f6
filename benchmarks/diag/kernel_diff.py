"""Compare the gfx950 code of the same kernels in two source trees (no GPU, no extension import).

    python benchmarks/diag/kernel_diff.py OLD_DIR NEW_DIR a.hip b.hip ... [--map OLD=NEW[:EXTRA]]

Each listed .hip of both directories is compiled to assembly with csrc/build.py's flags (FILE_FLAGS
included) plus -Rpass-analysis=kernel-resource-usage.  Kernels are matched across the trees by
their demangled name and template arguments; ``--map OLD=NEW:EXTRA`` says that OLD<args> of the old
tree is NEW<args, EXTRA> in the new one (a kernel folded into another under one more template
parameter), ``--map OLD=NEW`` a plain rename.  Per kernel it prints, as a markdown table, the
compiler's figures of both sides -- SGPRs, VGPRs, AGPRs, scratch bytes per lane, SGPR and VGPR
spills, occupancy, LDS bytes -- and whether the instruction streams are identical once mangled
names and the function number of .LBB labels are normalised; where they are not, the first and
last differing positions and both lengths.  Exit status 1 if any figure differs or a kernel has no
partner.
"""
from __future__ import annotations

import argparse
import importlib.util
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
_spec = importlib.util.spec_from_file_location("symb_build", ROOT / "csrc" / "build.py")
build = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(build)

FIGS = [("SGPRs", "sgpr"), ("VGPRs", "vgpr"), ("AGPRs", "agpr"), ("ScratchSize [bytes/lane]", "scr"),
        ("SGPRs Spill", "s_sp"), ("VGPRs Spill", "v_sp"), ("Occupancy [waves/SIMD]", "occ"),
        ("LDS Size [bytes/block]", "lds")]


def compile_one(src_dir: Path, name: str, tmp: Path):
    """-> {mangled kernel name: (figures dict, [normalised instructions])}"""
    out = tmp / (src_dir.name + "_" + str(abs(hash(str(src_dir)))) + "_" + Path(name).stem + ".s")
    cmd = [build.HIPCC, f"--offload-arch={build.ARCH}", "-O3", "-std=c++17", "-fPIC",
           "-fvisibility=hidden", "-Wno-unused-result", f"-I{src_dir}",
           *build.FILE_FLAGS.get(name, []), "--cuda-device-only", "-S",
           "-Rpass-analysis=kernel-resource-usage", str(src_dir / name), "-o", str(out)]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    if proc.returncode != 0:
        sys.exit(" ".join(cmd) + "\n" + proc.stderr)
    figs, cur = {}, None
    for line in proc.stderr.splitlines():
        m = re.search(r"remark:\s+(.+?):\s+(\S+)\s+\[-Rpass-analysis", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = figs.setdefault(m.group(2), {})
        elif cur is not None:
            cur[m.group(1).replace("TotalSGPRs", "SGPRs")] = m.group(2)   # (name varies by LLVM)
    streams, cur = {}, None
    for line in out.read_text().splitlines():
        m = re.match(r"(\w+):", line)
        if m and m.group(1) in figs:
            cur = streams.setdefault(m.group(1), [])
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None and line.startswith("\t") and line[1:2] not in (".", ";", ""):
            ins = re.sub(r"\s+", " ", line.split(";")[0].strip())
            ins = re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"_Z\w+", "SYM", ins))
            cur.append(ins)
    return {k: (figs[k], streams.get(k, [])) for k in figs}


def keyed(kernels: dict, maps: dict) -> dict:
    """mangled -> (name, template args) keys, old-tree names taken through ``maps``"""
    names = list(kernels)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True,
                         check=True).stdout.splitlines()
    out = {}
    for mangled, d in zip(names, dem):
        d = re.sub(r"^void ", "", d)
        d = re.sub(r"\(.*\)$", "", d).replace("symb::", "")
        base, _, targs = d.partition("<")
        targs = targs[:-1] if targs.endswith(">") else targs
        if base in maps:
            base, extra = maps[base]
            targs = ", ".join(x for x in (targs, extra) if x)
        out[(base, targs)] = kernels[mangled]
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old_dir", type=Path)
    ap.add_argument("new_dir", type=Path)
    ap.add_argument("files", nargs="+")
    ap.add_argument("--map", action="append", default=[], metavar="OLD=NEW[:EXTRA]")
    ap.add_argument("-j", type=int, default=8)
    a = ap.parse_args()
    maps = {}
    for m in a.map:
        old, _, new = m.partition("=")
        new, _, extra = new.partition(":")
        maps[old] = (new, extra)
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(a.j) as ex:
        jobs = [(d, f) for f in a.files for d in (a.old_dir, a.new_dir) if (d / f).exists()]
        res = list(ex.map(lambda j: compile_one(j[0].resolve(), j[1], Path(tmp)), jobs))
    old, new = {}, {}
    for (d, _), r in zip(jobs, res):
        (old if d is a.old_dir else new).update(r)
    old, new = keyed(old, maps), keyed(new, {})
    hdr = " / ".join(s for _, s in FIGS)
    print(f"| kernel | old: {hdr} | new | figures | stream |\n|---|---|---|---|---|")
    bad = 0
    for key in sorted(set(old) | set(new)):
        name = f"`{key[0]}<{key[1]}>`" if key[1] else f"`{key[0]}`"
        if key not in old or key not in new:
            print(f"| {name} | {'-' if key not in old else 'present'} | "
                  f"{'-' if key not in new else 'present'} | unmatched | |")
            bad += 1
            continue
        (fo, so), (fn, sn) = old[key], new[key]
        vo, vn = [fo.get(k, "?") for k, _ in FIGS], [fn.get(k, "?") for k, _ in FIGS]
        if so == sn:
            stream = f"identical ({len(so)})"
        else:
            first = next((i for i, (x, y) in enumerate(zip(so, sn)) if x != y), min(len(so), len(sn)))
            tail = next((i for i, (x, y) in enumerate(zip(so[::-1], sn[::-1])) if x != y),
                        min(len(so), len(sn)))
            stream = (f"differ: first at {first}, last at {len(so) - 1 - tail} / "
                      f"{len(sn) - 1 - tail}, lengths {len(so)} / {len(sn)}")
            if len(so) == len(sn):
                stream += f", {sum(x != y for x, y in zip(so, sn))} positions"
        bad += vo != vn
        print(f"| {name} | {' / '.join(vo)} | {' / '.join(vn)} | "
              f"{'same' if vo == vn else 'DIFFER'} | {stream} |")
    print(f"\n{len(set(old) | set(new))} kernels, {bad} with differing figures or unmatched")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
