#!/usr/bin/env python3
"""Build the reference MPI program as one-rank binaries, and record what they write.

    python oracle/build_ref.py            # oracle/_ref/mpi_<case>, one per case of the manifest
    python oracle/build_ref.py --record   # also run them and (re)write tests/golden/mpi_ref/

The manifest is tests/golden/mpi_ref/cases.json (settings only).  Every case
compiles the reference's own source file, in place in the reference checkout,
against the one-rank MPI of oracle/mpi_stub/ with the case's -D defines:

    cc -std=gnu11 -O2 -fwrapv -ffp-contract=off -I oracle/mpi_stub -D... SRC -o oracle/_ref/mpi_<case>

(-std=gnu11: the program declares functions without prototypes, which newer
default dialects reject; it changes no arithmetic.  -ffp-contract=off: no fused
multiply-add where the source has a product and a sum.)  One OpenMP twin
(-fopenmp -DOMPCH -DTHREAD_COUNT=4) of the manifest's "omp_twin" case is built
too.  Nothing of the reference is copied into this tree: only the binaries
under oracle/_ref/ (ignored by git) and, with --record, the files the binaries
write while they run.

The reference checkout is $HEAT_REFERENCE_DIR, by default the directory
`reference` next to this repository.  Where it does not exist the script says
so in one line and succeeds, leaving oracle/_ref/ as it is; it never fetches
anything.  Where it exists, a compile failure is an error.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ORACLE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(ORACLE)
STUB = os.path.join(ORACLE, "mpi_stub")
OUT = os.path.join(ORACLE, "_ref")
GOLDEN = os.path.join(ROOT, "tests", "golden", "mpi_ref")
MANIFEST = os.path.join(GOLDEN, "cases.json")
FILES = ("initial_im.dat", "final_im.dat")
ELAPSED = re.compile(r"^Elapsed time [0-9]+\.[0-9]+ secs$")
MAX_GOLDEN_BYTES = 100 * 1000


def reference_dir() -> str:
    return os.environ.get("HEAT_REFERENCE_DIR") or os.path.join(os.path.dirname(ROOT), "reference")


def manifest() -> dict:
    with open(MANIFEST) as f:
        return json.load(f)


def define_flags(defines: dict) -> list:
    return ["-D" + k if v is None else f"-D{k}={v}" for k, v in defines.items()]


def targets(m: dict) -> list:
    """(binary name, case, extra flags) of every binary, the OpenMP twin last."""
    t = [("mpi_" + c["name"], c, []) for c in m["cases"]]
    twin = m.get("omp_twin")
    if twin:
        of = next(c for c in m["cases"] if c["name"] == twin["of"])
        t.append(("mpi_" + twin["name"], of, list(twin["cflags"])))
    return t


def build(verbose: bool = True) -> bool:
    """Compile every binary; False (and nothing done) without a reference checkout."""
    ref = reference_dir()
    m = manifest()
    src = os.path.join(ref, m["program"])
    if not os.path.isfile(src):
        print(f"oracle: no reference checkout at {ref}: reference binaries not built")
        return False
    cc = os.environ.get("CC") or shutil.which("gcc") or "cc"
    os.makedirs(OUT, exist_ok=True)
    for name, case, extra in targets(m):
        out = os.path.join(OUT, name)
        tmp = out + ".tmp"
        cmd = ([cc, "-std=gnu11"] + m["cflags"] + extra + ["-I", STUB] + define_flags(case["defines"])
               + [src, "-o", tmp, "-lm"])
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:
            sys.stderr.write(p.stderr)
            raise SystemExit(f"oracle: building {name} failed: {' '.join(cmd)}")
        os.replace(tmp, out)
        if verbose:
            print(f"oracle: built {os.path.relpath(out, ROOT)}")
    return True


def run_binary(path: str, cwd: str) -> str:
    """Run a reference binary in `cwd`; its stdout.  It writes FILES there."""
    p = subprocess.run([path], cwd=cwd, capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        raise SystemExit(f"oracle: {path} exited {p.returncode}: {p.stderr}")
    return p.stdout


def same_but_elapsed(a: str, b: str) -> bool:
    la, lb = a.splitlines(), b.splitlines()
    return len(la) == len(lb) and all(x == y or (ELAPSED.match(x) and ELAPSED.match(y))
                                      for x, y in zip(la, lb))


def write_if_changed(path: str, data: bytes) -> None:
    if os.path.isfile(path):
        with open(path, "rb") as f:
            if f.read() == data:
                return
    with open(path, "wb") as f:
        f.write(data)
    print(f"oracle: wrote {os.path.relpath(path, ROOT)} ({len(data)} bytes)")


def digest_of(case: dict, files: dict) -> dict:
    """The golden of a case too large to commit: SHA-256 and length of both
    files and the manifest's sample lines (1-based) of final_im.dat, at least
    two of which must hold a negative value."""
    d = {"files": {k: {"sha256": hashlib.sha256(v).hexdigest(), "bytes": len(v)}
                   for k, v in files.items()}}
    lines = files["final_im.dat"].decode("ascii").split("\n")
    d["final_lines"] = {str(n): lines[n - 1] for n in case["sample_lines"]}
    if len(d["final_lines"]) != 4 or sum("-" in v for v in d["final_lines"].values()) < 2:
        raise SystemExit(f"oracle: {case['name']}: sample_lines must name four lines of "
                         "final_im.dat, two or more with a negative value")
    return d


def record() -> None:
    m = manifest()
    for case in m["cases"]:
        binary = os.path.join(OUT, "mpi_" + case["name"])
        with tempfile.TemporaryDirectory() as tmp:
            stdout = run_binary(binary, tmp)
            files = {}
            for k in FILES:
                with open(os.path.join(tmp, k), "rb") as f:
                    files[k] = f.read()
        gdir = os.path.join(GOLDEN, case["name"])
        os.makedirs(gdir, exist_ok=True)
        # The elapsed time differs from run to run: a recorded stdout that
        # differs from this run's in nothing else stays as it is.
        spath = os.path.join(gdir, "stdout.txt")
        old = open(spath).read() if os.path.isfile(spath) else None
        if old is None or not same_but_elapsed(old, stdout):
            write_if_changed(spath, stdout.encode())
        if case["golden"] == "digest":
            text = json.dumps(digest_of(case, files), indent=1) + "\n"
            write_if_changed(os.path.join(gdir, "digest.json"), text.encode())
        else:
            for k, v in files.items():
                if len(v) > MAX_GOLDEN_BYTES:
                    raise SystemExit(f"oracle: {case['name']}/{k} is {len(v)} bytes: too large to "
                                     "commit, make it a digest case")
                write_if_changed(os.path.join(gdir, k), v)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--record", action="store_true",
                    help="run every binary and (re)write the goldens under tests/golden/mpi_ref/")
    ap.add_argument("--quiet", action="store_true", help="one line per failure only")
    a = ap.parse_args(argv)
    built = build(verbose=not a.quiet)
    if a.record:
        if not built:
            raise SystemExit("oracle: --record needs the reference checkout")
        record()
    return 0


if __name__ == "__main__":
    sys.exit(main())
