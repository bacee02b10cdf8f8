"""Every kernel at byte offsets past 2^31, 2^32, 2^33 and 2^34 from its origin
pointer (signed / unsigned 32-bit byte offsets and float indices), against the
windowed NumPy oracle of tests/large_cases.py.  Needs an MI355X.

A. Sub-box runs: the fields are poisoned (source NaN outside the band's light
   cone, destination a sentinel) and each kernel runs on a 64-row band around
   each mark, and on the plate's first and last rows: every offset inside the
   kernel is large, the work is 0.26 M cells.  Bitwise against the oracle, and
   nothing outside the band written.
B. Whole-plate runs (planner scale, grid sizes, unit counts): with zero
   coefficients every kernel must return its source (every centre load and
   store of every row), with the default ones the bands must equal the oracle.
C. The service kernels that take a whole field, on the 1,000,000-row plate.
D. One solver run against 36 whole-plate naive steps.

One field set lives at a time (module-scoped fixture, freed at teardown), at
most 36 GiB of device memory; no copy to the host is larger than a band, whole
fields are compared by reductions on the device."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from parallel_heat_amd import HeatConfig, HeatSolver, ops
from parallel_heat_amd.models import reference as R
from parallel_heat_amd.parallel.topology import layout

from . import large_cases as LC
from . import refine_cases as RC
from . import service_cases as SC

pytestmark = pytest.mark.gpu

V = ops.TbVariant
DEF = V.DEFAULT
DEEP = V.DEFAULT_DEEP
TILE = V.TILE | V.XCD_GROUPS
SEED, QSEED = 29, 7
GIB = 1 << 30
BUDGET = 36 * GIB
# Fields per set (SOLVER: two reference fields next to a solver's own two).
COUNT = {"DEEP": 2, "MID3": 3, "SQUARE": 4, "WIDE": 2, "CELLS": 2, "SOLVER": 4}
PLATES = dict(LC.SETS, SOLVER=LC.SETS["SQUARE"])
LABELS = {1 << 31: "2^31B", 1 << 32: "2^32B", 1 << 33: "2^33B", 1 << 34: "2^34B"}


def _labelled_bands(f, width):
    """{"first", "2^31B", ..., "last"} -> box; no two of them overlap."""
    out = {}
    for m, r, c in LC.marks(f):
        first, band, last = LC.bands(f, [(m, r, c)], width=width)
        out[LABELS[m]] = band
    out = dict(first=first, **out, last=last)
    rows = sorted((b[0], b[1]) for b in out.values())
    assert all(p[1] <= n[0] for p, n in zip(rows, rows[1:])), out
    return out


@pytest.fixture(scope="module")
def fs(request):
    """The field set named by the (indirect) parameter: allocated once, freed
    before the next one is built."""
    name = request.param
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    nx, ny = PLATES[name]
    pitch, rows, _, _ = layout(nx, ny, LC.HALO)  # recomputed, not hard-coded
    need = COUNT[name] * pitch * rows * 4 + GIB  # + the reductions' temporaries
    assert need <= BUDGET, (name, need)
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info()[0]
    if free < need:
        pytest.skip(f"{name}: needs {need / GIB:.1f} GiB of free device memory, "
                    f"{free / GIB:.1f} GiB are free")
    torch.cuda.reset_peak_memory_stats()
    n = 2 if name == "SOLVER" else COUNT[name]
    s = SimpleNamespace(name=name, nx=nx, ny=ny, dev=dev, cache={},
                        fields=[ops.Field(nx, ny, LC.HALO, dev) for _ in range(n)])
    s.bands = _labelled_bands(s.fields[0], None if ny <= 8192 else 1024)
    yield s
    # Freed for certain: the report of a failed test keeps its frame, and with
    # it the fields, alive.
    for f in s.fields:
        f.data.untyped_storage().resize_(0)
    s.fields.clear()
    s.cache.clear()
    del s
    torch.cuda.empty_cache()
    peak = torch.cuda.max_memory_allocated()
    print(f"\n{name}: peak device memory {peak / GIB:.2f} GiB")
    assert peak <= BUDGET, (name, peak)


def on(name):
    return pytest.mark.parametrize("fs", [name], indirect=True)


MID3_BANDS = ("first", "2^31B", "2^32B", "2^33B", "last")


def band_param(*names):
    """One case per band of the set: the rows at each mark, the first, the last."""
    return pytest.mark.parametrize(
        "band", list(names) or ["first", "2^31B", "2^32B", "2^33B", "2^34B", "last"])


@pytest.fixture
def tuning():
    """Set TbTuning fields for one test, restore after."""
    saved = ops.tb_tuning()

    def set_(**kw):
        t = ops.tb_tuning()
        for k, v in kw.items():
            assert hasattr(t, k), k
            setattr(t, k, v)
        ops.set_tb_tuning(t)

    yield set_
    ops.set_tb_tuning(saved)


def levels(s, box, k=12, q=None, cx=0.1, cy=0.1, step=R.step_np_fma):
    """Oracle states 0..k of `box`, computed once per set.  States up to 12
    come from one window grown by 12: a wider window than a state needs gives
    the same bits (test_large_cases_cpu.py checks every state of it)."""
    key = (box, k, q, cx, cy, step.__name__)
    if key not in s.cache:
        s.cache[key] = LC.window_levels(s.nx, s.ny, SEED, box, k, cx, cy, q, step)
    return s.cache[key]


def geom(s, cx=0.1, cy=0.1):
    return ops.Geom(nx=s.nx, ny=s.ny, cx=cx, cy=cy)


def host(f, box):
    return f.view(*box).cpu().numpy()


def check_band(s, dst, box, want, what):
    torch.cuda.synchronize()
    SC.assert_same_bits(host(dst, box), want, f"{s.name} {what} {box}")
    assert LC.untouched(dst, [box]) == 0, f"{s.name} {what} {box}: stores outside the box"


# ---------------------------------------------------------------------------
# A. sub-box runs at every mark
# ---------------------------------------------------------------------------
@on("DEEP")
@band_param()
def test_naive_step_band(fs, band):
    a, b = fs.fields
    box = fs.bands[band]
    LC.poison(a, b, [box], 1, SEED)
    ops.naive_step(a, b, geom(fs), box)
    check_band(fs, b, box, levels(fs, box)[1], "naive")


@on("DEEP")
@band_param()
@pytest.mark.parametrize("numerics", ["fp32", "mpi"])
def test_lds_step_band(fs, band, numerics):
    a, b = fs.fields
    box = fs.bands[band]
    LC.poison(a, b, [box], 1, SEED)
    ops.lds_step(a, b, geom(fs), box, numerics=numerics)
    want = levels(fs, box)[1] if numerics == "fp32" else levels(fs, box, 1, step=R.step_np_mpi)[1]
    check_band(fs, b, box, want, f"lds {numerics}")


@on("DEEP")
@band_param()
def test_mfma_step_band_exact_chain(fs, band):
    # The kernel's own association (LC.step_np_mfma), bit for bit: as sharp at
    # these offsets as the other kernels' checks.
    a, b = fs.fields
    box = fs.bands[band]
    LC.poison(a, b, [box], 1, SEED)
    ops.mfma_step(a, b, geom(fs), box)
    check_band(fs, b, box, levels(fs, box, 1, step=LC.step_np_mfma)[1], "mfma")


@on("DEEP")
@band_param()
def test_mfma_step_band(fs, band):
    """Against the canonical oracle within the bound of
    test_mfma_step_close_to_oracle, 2e-5.  With the centre term second in
    the kernel's fmaf chain, five of the six bands of 260,608 cells held a
    cell three ulps of [64, 128) away, 2.289e-05 (the 104,951 cells of that
    test hold none); the chain now adds the neighbours first and the centre
    last, which keeps it within 1.87e-5 of heat::stencil on such values
    (LC.step_np_mfma has the reckoning)."""
    a, b = fs.fields
    box = fs.bands[band]
    LC.poison(a, b, [box], 1, SEED)
    ops.mfma_step(a, b, geom(fs), box)
    torch.cuda.synchronize()
    got, ref = host(b, box), levels(fs, box)[1]
    err = float(np.abs(got - ref).max())
    print(f"mfma {band}: max |got - oracle| = {err:.3e}")
    SC.assert_same_bits(got[:, 0], ref[:, 0], "west ring")
    SC.assert_same_bits(got[:, -1], ref[:, -1], "east ring")
    if band == "first":
        SC.assert_same_bits(got[0], ref[0], "north ring")
    if band == "last":
        SC.assert_same_bits(got[-1], ref[-1], "south ring")
    assert LC.untouched(b, [box]) == 0
    assert err <= 2e-5  # (a NaN fails it)


TB_CASES = [("DEF@8", DEF, 8, {}), ("DEF@12", DEF, 12, {}),
            ("DEF|ALT@12", DEF | V.ALT_DIRECTION, 12, {}),
            ("DEEP@8", DEEP, 8, {}), ("DEEP@12", DEEP, 12, {}),
            ("DEEP@12,nt=1", DEEP, 12, dict(nt=1)),
            ("DEEP|LINEAR@12", DEEP | V.LINEAR, 12, {}),
            ("TILE12x8@12", TILE, 12, dict(tile_rows=12, tile_waves=8)),
            ("TILE@8,xl=1", TILE, 8, dict(tile_xl=1))]


@on("DEEP")
@band_param()
@pytest.mark.parametrize("case", TB_CASES, ids=[c[0] for c in TB_CASES])
def test_tb_step_band(fs, tuning, band, case):
    what, variant, k, knobs = case
    a, b = fs.fields
    box = fs.bands[band]
    tuning(**knobs)
    LC.poison(a, b, [box], k, SEED)
    ops.tb_step(a, b, geom(fs), k, boxes=[box], variant=int(variant))
    check_band(fs, b, box, levels(fs, box)[k], what)


@on("DEEP")
@band_param()
@pytest.mark.parametrize("res_level", [6, 0])
def test_tb_step_band_residual(fs, band, res_level):
    # As test_tb_inner_level_residual / test_tb_residual: the word is the
    # oracle's max |u_rl - u_(rl-1)| over the band, the 12-step state intact.
    a, b = fs.fields
    box = fs.bands[band]
    LC.poison(a, b, [box], 12, SEED)
    resid = torch.zeros(1, dtype=torch.int32, device=fs.dev)
    ops.tb_step(a, b, geom(fs), 12, boxes=[box], resid=resid, variant=int(DEEP),
                res_level=res_level)
    lv = levels(fs, box)
    check_band(fs, b, box, lv[12], f"DEEP@12 res_level={res_level}")
    rl = res_level or 12
    want = float(np.abs(lv[rl] - lv[rl - 1]).max())
    assert ops.resid_value(resid) == want, (ops.resid_value(resid), want)


@on("DEEP")
@band_param()
def test_residual_band(fs, band):
    # a: the initial condition on the band alone, b: the sentinel; a read
    # outside the band meets a NaN, which wins the unsigned maximum.
    a, b = fs.fields
    box = fs.bands[band]
    LC.poison(a, b, [box], 0, SEED)
    want = float(np.abs(LC.init_window(fs.nx, fs.ny, SEED, box) - np.float32(LC.SENTINEL)).max())
    assert ops.residual(a, b, box) == want
    assert ops.residual(b, a, box) == want


@on("DEEP")
def test_pack_unpack_copy_boxes_bands(fs):
    a, b = fs.fields
    boxes = list(fs.bands.values())
    LC.poison(a, b, boxes, 0, SEED)
    init = [LC.init_window(fs.nx, fs.ny, SEED, box) for box in boxes]
    bufs = [torch.full((SC.box_size(box),), 7.0, device=fs.dev) for box in boxes]
    for box, buf, want in zip(boxes, bufs, init):
        ops.pack(a, box, buf)
        torch.cuda.synchronize()
        SC.assert_same_bits(buf.cpu().numpy().reshape(want.shape), want, f"pack {box}")
        ops.unpack(buf, b, box)
    torch.cuda.synchronize()
    for box, want in zip(boxes, init):
        SC.assert_same_bits(host(b, box), want, f"unpack {box}")
    assert LC.untouched(b, boxes) == 0
    # The same through the one-launch copy of up to 8 boxes, both ways.
    b.data.fill_(LC.SENTINEL)
    bufs2 = [torch.full_like(buf, 9.0) for buf in bufs]
    ops.copy_boxes(a, list(zip(boxes, bufs2)), to_buf=True)
    ops.copy_boxes(b, list(zip(boxes, bufs2)), to_buf=False)
    torch.cuda.synchronize()
    for box, buf, want in zip(boxes, bufs2, init):
        SC.assert_same_bits(buf.cpu().numpy().reshape(want.shape), want, f"copy_boxes {box}")
        SC.assert_same_bits(host(b, box), want, f"copy_boxes back {box}")
    assert LC.untouched(b, boxes) == 0


# ---------------------------------------------------------------------------
# B. whole-plate runs
# ---------------------------------------------------------------------------
def _run(kernel, a, b, g, q=None):
    if kernel == "naive":
        ops.naive_step(a, b, g)
        return 1
    if kernel == "lds":
        ops.lds_step(a, b, g)
        return 1
    if kernel == "source":
        ops.source_step(a, b, q, g)
        return 1
    name, k = kernel.split("@")
    ops.tb_step(a, b, g, int(k), variant={"tb": -1, "linear": int(DEEP | V.LINEAR)}[name])
    return int(k)


def _whole_plate(s, kernel, check):
    a, b = s.fields[:2]
    q = None
    ops.init_field(a, ops.Geom(nx=s.nx, ny=s.ny), "random", SEED)
    b.data.fill_(LC.SENTINEL)
    if kernel == "source":
        q = s.fields[2]
        if check == "identity":
            q.data.zero_()
        else:  # source_window, computed on the device in the same two fp32 operations
            ops.init_field(q, ops.Geom(nx=s.nx, ny=s.ny), "random", QSEED ^ 0x5EED)
            q.data.sub_(50.0).mul_(0.03125)
    if check == "identity":
        # cx = cy = 0: every step returns its source, and the random plate
        # holds no zero: this sees every centre load and store of every row.
        _run(kernel, a, b, geom(s, 0.0, 0.0), q)
        torch.cuda.synchronize()
        assert LC.same_values(b.owned(), a.owned()), f"{s.name} {kernel}: dst != src"
        # ... and nothing but the owned block was written.
        assert LC.count_ne(b.data, LC.SENTINEL) == s.nx * s.ny
        return
    k = _run(kernel, a, b, geom(s), q)
    torch.cuda.synchronize()
    for label, box in s.bands.items():
        lv = levels(s, box, 8, q=QSEED) if kernel == "source" else levels(s, box)
        SC.assert_same_bits(host(b, box), lv[k], f"{s.name} {kernel} band {label} {box}")


CHECKS = ["identity", "bands"]
PLATE_KERNELS = ["naive", "lds", "tb@8", "tb@12", "linear@12"]


@on("DEEP")
@pytest.mark.parametrize("check", CHECKS)
@pytest.mark.parametrize("kernel", ["naive", "lds", "tb@12"])
def test_whole_plate_deep(fs, kernel, check):
    # naive: 250,000 rows of blocks in y, above the 65,535 of a launch's grid.
    _whole_plate(fs, kernel, check)


# ---------------------------------------------------------------------------
# C. service kernels on the whole 1,000,000-row block (before the other plates
# of B: one field set lives at a time)
# ---------------------------------------------------------------------------
def _banded(s, f):
    """f: 0.0 everywhere but the bands, which hold the random plate; the host
    copies of the bands."""
    f.data.zero_()
    out = {}
    for label, box in s.bands.items():
        out[label] = LC.init_window(s.nx, s.ny, SEED, box)
        f.view(*box).copy_(torch.from_numpy(out[label]))
    return out


@on("DEEP")
def test_init_field_bands(fs):
    a = fs.fields[0]
    a.data.fill_(LC.SENTINEL)
    ops.init_field(a, geom(fs), "random", SEED)
    torch.cuda.synchronize()
    for label, box in fs.bands.items():
        SC.assert_same_bits(host(a, box), LC.init_window(fs.nx, fs.ny, SEED, box), label)
    # Every cell of the tensor was written (no value of the plate is negative).
    assert LC.count_ne(a.data, LC.SENTINEL) == a.rows * a.pitch
    assert all(float(c.min()) >= 0.0 for c in LC.chunks(a.owned()))


class _Rows:
    """Rows [r0, r1) of a field as a field of their own (what ops.checksum reads)."""

    def __init__(self, f, r0, r1):
        self.f, self.r0, self.lx, self.ly, self.pitch, self.device = f, r0, r1 - r0, f.ly, f.pitch, f.device

    def ptr(self):
        return self.f.ptr() + 4 * self.r0 * self.pitch


@on("DEEP")
def test_checksum_whole_block(fs):
    a = fs.fields[0]
    vals = _banded(fs, a)
    whole = ops.checksum(a)
    assert whole["count"] == fs.nx * fs.ny
    own = a.owned()
    chunks = LC.chunks(own)
    assert whole["min"] == min(float(c.amin()) for c in chunks) == 0.0
    assert whole["max"] == max(float(c.amax()) for c in chunks)
    assert whole["max"] == max(float(v.max()) for v in vals.values())
    # Zeros add exactly: the exact sum and the bound are those of the bands.
    flat = np.concatenate([v.ravel() for v in vals.values()])
    exact, bound = math.fsum(flat.astype(np.float64).tolist()), SC.sum_bound(flat)
    dsum = sum(float(c.sum(dtype=torch.float64)) for c in chunks)
    print(f"checksum sum: |kernel - fsum| {abs(whole['sum'] - exact):.3e}, |torch - fsum| "
          f"{abs(dsum - exact):.3e}, bound {bound:.3e}")
    assert abs(whole["sum"] - exact) <= bound and abs(dsum - exact) <= bound
    # hash: the blocks' hashes taken at their offsets add up (check_decomposition),
    # every block below 2^31 bytes; the bands are blocks of their own, held to
    # reference.checksum_np.
    step = ((1 << 31) - 1) // (4 * a.pitch)
    cuts = sorted({0, fs.nx} | {r for b in fs.bands.values() for r in b[:2]})
    blocks = [(r, min(r + step, hi)) for lo, hi in zip(cuts, cuts[1:]) for r in range(lo, hi, step)]
    assert all((r1 - r0) * a.pitch * 4 < 1 << 31 for r0, r1 in blocks)
    by_rows = {box[:2]: label for label, box in fs.bands.items()}
    parts = []
    for r0, r1 in blocks:
        c = ops.checksum(_Rows(a, r0, r1), r0, 0, fs.ny)
        if (r0, r1) in by_rows:
            SC.assert_checksum(c, vals[by_rows[(r0, r1)]], r0, 0, fs.ny, what=by_rows[(r0, r1)])
        else:
            assert c["min"] == c["max"] == c["sum"] == 0.0
        parts.append(c)
    assert sum(c["hash"] for c in parts) & SC.M64 == whole["hash"]
    assert sum(c["count"] for c in parts) == whole["count"]


@on("DEEP")
@pytest.mark.parametrize("mode", ["mirror", "wrap"])
def test_fill_edge_ghosts_whole_block(fs, mode):
    a = fs.fields[0]
    vals = _banded(fs, a)
    k, lx, ly = LC.HALO, fs.nx, fs.ny
    ops.fill_edge_ghosts(a, *(("all", "") if mode == "mirror" else ("", "xy")), k)
    torch.cuda.synchronize()
    pad = dict(mode="reflect" if mode == "mirror" else "wrap")
    for label, box in fs.bands.items():  # W / E ghost columns of the band's rows
        want = np.pad(vals[label], ((0, 0), (k, k)), **pad)
        SC.assert_same_bits(host(a, (box[0], box[1], -k, ly + k)), want, f"{mode} W/E {label}")
    if mode == "mirror":  # the S / N ghost rows with their corners
        south = np.pad(np.pad(vals["last"], ((0, k), (0, 0)), **pad), ((0, 0), (k, k)), **pad)[-k:]
        north = np.pad(np.pad(vals["first"], ((k, 0), (0, 0)), **pad), ((0, 0), (k, k)), **pad)[:k]
    else:
        south = np.pad(vals["first"][:k], ((0, 0), (k, k)), **pad)
        north = np.pad(vals["last"][-k:], ((0, 0), (k, k)), **pad)
    SC.assert_same_bits(host(a, (lx, lx + k, -k, ly + k)), south, f"{mode} S ghost rows")
    SC.assert_same_bits(host(a, (-k, 0, -k, ly + k)), north, f"{mode} N ghost rows")
    # Owned cells are as they were.
    for label, box in fs.bands.items():
        SC.assert_same_bits(host(a, box), vals[label], f"{mode} owned {label}")


@on("DEEP")
@pytest.mark.parametrize("fx,fy", [(64, 64), (1000, 1000)])
def test_coarse_whole_block(fs, fx, fy):
    # 64 x 64: a coarse cell inside one wave's share; 1000 x 1000: cut across waves.
    a = fs.fields[0]
    vals = _banded(fs, a)
    out = ops.coarse(a, fx, fy)
    torch.cuda.synchronize()
    cr, cc = ops.coarse_dims(fs.nx, fs.ny, fx, fy)
    want = LC.coarse_banded([(fs.bands[label][0], v) for label, v in vals.items()],
                            fs.nx, fs.ny, fx, fy)
    idx = torch.tensor(sorted(want), device=fs.dev)
    got = {k: out[k][idx].cpu().numpy() for k in ("sum", "min", "max")}
    for n, i in enumerate(sorted(want)):
        s, mn, mx, bound = want[i]
        assert np.array_equal(got["min"][n], mn) and np.array_equal(got["max"][n], mx), (i, fx, fy)
        assert (np.abs(got["sum"][n] - s) <= bound).all(), (i, np.abs(got["sum"][n] - s), bound)
    rest = torch.ones(cr, dtype=torch.bool, device=fs.dev)
    rest[idx] = False
    for k in ("sum", "min", "max"):  # every other coarse cell: all zeros
        assert int((out[k][rest] != 0).sum()) == 0, k
    rows = np.minimum(np.arange(1, cr + 1) * fx, fs.nx) - np.arange(cr) * fx
    cols = np.minimum(np.arange(1, cc + 1) * fy, fs.ny) - np.arange(cc) * fy
    assert np.array_equal(out["count"].numpy(), rows[:, None] * cols[None, :])
    assert int(out["count"].sum()) == fs.nx * fs.ny


@on("DEEP")
@pytest.mark.parametrize("order", [0, 1])
def test_refine_whole_block(fs, order):
    a = fs.fields[0]
    fx, fy = 1000, 64
    S = RC.source("int", -(-fs.nx // fx), -(-fs.ny // fy))
    a.data.fill_(LC.SENTINEL)
    ops.refine(a, S, fx, fy, order=order)
    torch.cuda.synchronize()
    for label, (r0, r1, c0, c1) in fs.bands.items():
        want = LC.refine_rows(S, fs.nx, fs.ny, fx, fy, order, r0, r1)
        SC.assert_same_bits(host(a, (r0, r1, 0, fs.ny)), want, f"refine order {order} {label}")
    assert LC.untouched(a, [(0, fs.nx, 0, fs.ny)]) == 0  # owned cells alone
    if order == 0:  # ... and every one of them: the source holds integers
        assert LC.count_ne(a.data, LC.SENTINEL) == fs.nx * fs.ny


# ---------------------------------------------------------------------------
# A, continued: the source kernels (three fields: the half-height plate)
# ---------------------------------------------------------------------------
@pytest.fixture
def source_nt():
    yield ops.set_source_nontemporal
    ops.set_source_nontemporal(-1)


@on("MID3")
@band_param(*MID3_BANDS)
@pytest.mark.parametrize("nt", [1, 0])
def test_source_step_band(fs, source_nt, band, nt):
    a, b, q = fs.fields
    box = fs.bands[band]
    source_nt(nt)
    LC.poison(a, b, [box], 1, SEED, q=q, qseed=QSEED, grow_q=0)
    ops.source_step(a, b, q, geom(fs), box)
    check_band(fs, b, box, levels(fs, box, 8, q=QSEED)[1], f"source nt={nt}")


@on("MID3")
@band_param(*MID3_BANDS)
@pytest.mark.parametrize("k", [2, 8])
def test_source_tb_step_band(fs, band, k):
    a, b, q = fs.fields
    box = fs.bands[band]
    LC.poison(a, b, [box], k, SEED, q=q, qseed=QSEED, grow_q=k - 1)
    ops.source_tb_step(a, b, q, geom(fs), box, k)
    check_band(fs, b, box, levels(fs, box, 8, q=QSEED)[k], f"source_tb k={k}")


# ---------------------------------------------------------------------------
# B, continued: the other plates
# ---------------------------------------------------------------------------
@on("SQUARE")
@pytest.mark.parametrize("check", CHECKS)
@pytest.mark.parametrize("kernel", PLATE_KERNELS + ["source"])
def test_whole_plate_square(fs, kernel, check):
    _whole_plate(fs, kernel, check)


@on("SQUARE")
@pytest.mark.parametrize("k", [8, 12])
def test_tb_equals_naive_steps_square(fs, k):
    # Four fields fit: the fused pass against k whole-plate naive steps, which
    # their own identity and band checks anchor.
    a, b, c, d = fs.fields
    g = geom(fs)
    for f in (a, c):
        ops.init_field(f, g, "random", SEED)
    b.data.fill_(LC.SENTINEL)
    ops.tb_step(a, b, g, k)
    for _ in range(k):
        ops.naive_step(c, d, g)
        c, d = d, c
    torch.cuda.synchronize()
    assert LC.same_values(b.owned(), c.owned())


@on("WIDE")
@pytest.mark.parametrize("check", CHECKS)
@pytest.mark.parametrize("kernel", PLATE_KERNELS)
def test_whole_plate_wide(fs, kernel, check):
    # The marks fall mid-row; more than 4,270 strips.
    _whole_plate(fs, kernel, check)


@on("CELLS")
@pytest.mark.parametrize("check", CHECKS)
def test_whole_plate_cells(fs, check):
    # More than 2^31 cells in one launch.
    _whole_plate(fs, "tb@12", check)


# ---------------------------------------------------------------------------
# D. one solver-level run
# ---------------------------------------------------------------------------
@on("SOLVER")
def test_solver_equals_whole_plate_naive_steps(fs):
    a, b = fs.fields
    g = geom(fs)
    ops.init_field(a, g, "random", SEED)
    ops.init_field(b, g, "random", SEED)
    for _ in range(36):
        ops.naive_step(a, b, g)
        a, b = b, a
    torch.cuda.synchronize()
    want = ops.checksum(a)
    cfg = HeatConfig(nx=fs.nx, ny=fs.ny, steps=36, init="random", seed=SEED, backend="hip",
                     device=0)
    assert cfg.use_graph and cfg.kernel == "auto"
    with HeatSolver(cfg) as solver:
        r = solver.run()
        got = solver.checksum()
        coarse = solver.coarse(1000)
    assert r.steps_done == 36
    assert int(got["hash"], 16) == want["hash"] and got["count"] == want["count"] == fs.nx * fs.ny
    cr = fs.nx // 1000
    blocks = [a.owned()[i * 1000:(i + 1) * 1000].reshape(1000, cr, 1000) for i in range(cr)]
    mn = torch.stack([t.amin(dim=(0, 2)) for t in blocks]).cpu().numpy()
    mx = torch.stack([t.amax(dim=(0, 2)) for t in blocks]).cpu().numpy()
    assert np.array_equal(np.asarray(coarse["min"]), mn)
    assert np.array_equal(np.asarray(coarse["max"]), mx)
