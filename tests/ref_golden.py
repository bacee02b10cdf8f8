"""Goldens recorded from the reference MPI program (tests/golden/mpi_ref/).

What the reference's own binary wrote, one rank against the one-rank MPI of
oracle/mpi_stub (oracle/build_ref.py --record): initial_im.dat, final_im.dat
and stdout per case of cases.json; the case too large to commit is a digest
(SHA-256, lengths, four whole lines).  Everything here reads tests/golden/
only, so it works where no reference checkout and no reference binary exists.

The reference prints the loop index `it` of its converging check; it has then
done it + 1 updates, the engine's converged_at.  A run that never converges
does STEPS + 1 updates.
"""
import hashlib
import json
import os
import re
import subprocess
import tempfile
from functools import lru_cache

from parallel_heat_amd import HeatConfig
from parallel_heat_amd.utils import io as hio
from parallel_heat_amd.utils import report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "mpi_ref")
REF_BIN = os.path.join(ROOT, "oracle", "_ref")
ELAPSED = re.compile(r"^Elapsed time \d+\.\d{6} secs$")
CONVERGED = re.compile(r"^Converged after (\d+) steps$")
# What every run of the reference program's role is configured with.
MPI_KW = dict(numerics="mpi", compat="mpi", init="ref-wrap")


class Case:
    def __init__(self, spec):
        self.name = spec["name"]
        self.defines = spec["defines"]
        self.config = dict(spec["config"])
        self.cli = list(spec["cli"])
        self.golden = spec["golden"]
        self.dir = os.path.join(GOLDEN, self.name)
        self.nx, self.ny, self.steps = (self.config[k] for k in ("nx", "ny", "steps"))
        self.converge = bool(self.config.get("converge", False))

    def __repr__(self):
        return f"Case({self.name})"

    def read(self, name):
        with open(os.path.join(self.dir, name), "rb") as f:
            return f.read()

    @property
    def lines(self):
        """The reference's stdout lines, as recorded."""
        return self.read("stdout.txt").decode("ascii").splitlines()

    @property
    def ref_it(self):
        """The step number the reference printed, None where it did not converge."""
        hits = [CONVERGED.match(l) for l in self.lines]
        hits = [int(m.group(1)) for m in hits if m]
        assert len(hits) <= 1
        if not hits:
            assert not self.converge or "Didn't converged" in self.lines
        return hits[0] if hits else None

    @property
    def total_steps(self):
        """Updates the reference did: it + 1 where it converged, else STEPS + 1."""
        return self.steps + 1 if self.ref_it is None else self.ref_it + 1

    @property
    def binary(self):
        return os.path.join(REF_BIN, "mpi_" + self.name)

    def heat_config(self, **kw):
        return HeatConfig(**{**self.config, **MPI_KW, **kw})


@lru_cache(maxsize=None)
def manifest():
    with open(os.path.join(GOLDEN, "cases.json")) as f:
        return json.load(f)


@lru_cache(maxsize=None)
def cases():
    return tuple(Case(c) for c in manifest()["cases"])


def case(name):
    return next(c for c in cases() if c.name == name)


def names(exclude=()):
    return [c.name for c in cases() if c.name not in exclude]


def normalised(lines):
    """stdout lines with the elapsed seconds, the one thing that differs from
    run to run, replaced; the line itself must have the reference's form."""
    out = []
    for l in lines:
        if l.startswith("Elapsed time"):
            assert ELAPSED.match(l), l
            l = "Elapsed time T secs"
        out.append(l)
    return out


def expected_lines(c, world=1):
    """The golden stdout for a run on `world` ranks: the reference prints its
    task count in the first line and nothing else depends on it."""
    lines = normalised(c.lines)
    assert lines[0] == "Starting mpi_heat2D with 1 worker tasks."
    lines[0] = f"Starting mpi_heat2D with {world} worker tasks."
    return lines


def assert_file(c, name, data):
    """`data` is byte for byte what the reference wrote as `name`."""
    if c.golden == "files":
        want = c.read(name)
        if data != want:
            n = next((i for i, (a, b) in enumerate(zip(data, want)) if a != b),
                     min(len(data), len(want)))
            line = want[:n].count(b"\n") + 1
            raise AssertionError(f"{c.name}/{name}: {len(data)} bytes vs the golden's {len(want)}, "
                                 f"first difference at byte {n} (line {line})")
        return
    d = json.loads(c.read("digest.json"))
    if name == "final_im.dat":  # the sampled lines first: they say where it differs
        lines = data.decode("ascii").split("\n")
        assert len(d["final_lines"]) == 4
        assert sum("-" in v for v in d["final_lines"].values()) >= 2
        for n, want in d["final_lines"].items():
            assert lines[int(n) - 1] == want, f"{c.name}/{name} line {n}"
    assert len(data) == d["files"][name]["bytes"], f"{c.name}/{name} length"
    assert hashlib.sha256(data).hexdigest() == d["files"][name]["sha256"], f"{c.name}/{name} SHA-256"


def dat_bytes(grid):
    """The grid as the engine's prtdat writer prints it."""
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "g.dat")
        hio.write_dat(p, grid)
        with open(p, "rb") as f:
            return f.read()


def assert_run(c, result, world=1):
    """A RunResult stopped where the reference did, and the lines the package
    prints for it are the reference's."""
    if c.ref_it is None:
        assert not result.converged, f"{c.name}: converged at {result.converged_at}, the reference never"
        assert result.steps_done == c.steps + 1
    else:
        assert result.converged, f"{c.name}: did not converge, the reference did at it={c.ref_it}"
        assert result.converged_at - 1 == c.ref_it
        assert result.steps_done == result.converged_at
    want = expected_lines(c, world)
    banner = report.mpi_banner(world, c.nx, c.ny, c.steps, c.converge)
    assert banner == "".join(l + "\n" for l in want[:2])
    if c.converge:
        line = report.convergence_line("mpi", result.converged, result.converged_at, c.steps)
        assert line == want[2] + "\n"
        assert len(want) == 4
    else:
        assert len(want) == 3
    assert want[-1] == "Elapsed time T secs"
    assert normalised([report.elapsed_line("mpi", result.seconds).rstrip("\n")])[0] == want[-1]


def assert_grid(c, grid):
    assert grid.shape == (c.nx, c.ny)
    assert_file(c, "final_im.dat", dat_bytes(grid))


def run_reference_binary(path, cwd):
    """(stdout lines, {file name: bytes}) of a reference binary run in `cwd`."""
    p = subprocess.run([path], cwd=cwd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    files = {}
    for k in ("initial_im.dat", "final_im.dat"):
        with open(os.path.join(cwd, k), "rb") as f:
            files[k] = f.read()
    return p.stdout.splitlines(), files
