"""The helpers of the large-offset GPU tests (tests/large_cases.py), held
honest where there is no GPU: the same harness against the CPU ops on a plate
of a few hundred rows with the marks scaled down into it, the marks and bands
against offsets computed from layout() alone, the windowed oracle against the
full-plate one, and the poisoning against deliberately misplaced accesses."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from parallel_heat_amd import ops
from parallel_heat_amd.models import reference as R
from parallel_heat_amd.parallel.topology import layout

from . import large_cases as LC
from . import refine_cases as RC
from . import service_cases as SC

NX, NY, SEED = 330, 600, 17
# Pitch 896: the marks fall at local cells (24, 500), (61, 116), (134, 244), (280, 500).
SMALL = (1 << 17, 1 << 18, 1 << 19, 1 << 20)


def _plate(device="cpu"):
    return ops.Field(NX, NY, LC.HALO, device), ops.Field(NX, NY, LC.HALO, device)


def _shape(nx, ny):
    pitch, rows, hx, hy = layout(nx, ny, LC.HALO)
    return SimpleNamespace(lx=nx, ly=ny, pitch=pitch, rows=rows, hx=hx, hy=hy)


def test_marks_are_the_cells_at_those_byte_offsets():
    a, _ = _plate()
    pitch, rows, hx, hy = layout(NX, NY, LC.HALO)
    got = LC.marks(a, SMALL)
    assert [m for m, _, _ in got] == list(SMALL)
    for m, r, c in got:
        assert ((r + hx) * pitch + (c + hy)) * 4 == m
        assert 0 <= r < NX and 0 <= c < NY  # owned cells, all four
        assert a.view(r, r + 1, c, c + 1).data_ptr() - a.data.data_ptr() == m
    # A mark beyond the tensor is left out.
    assert LC.marks(a, [rows * pitch * 4]) == []
    assert LC.marks(a, [rows * pitch * 4 - 4]) == [(rows * pitch * 4 - 4, NX + hx - 1, pitch - hy - 1)]


@pytest.mark.parametrize("width", [None, 64])
def test_bands_hold_the_marks_and_the_plate_ends(width):
    a, _ = _plate()
    ms = LC.marks(a, SMALL)
    bs = LC.bands(a, ms, half=8, width=width, edge=16)
    for r0, r1, c0, c1 in bs:
        assert 0 <= r0 < r1 <= NX and 0 <= c0 < c1 <= NY
        assert c0 % 4 == 0 and c1 % 4 == 0
        assert c1 - c0 == (NY if width is None else width)
    for _, r, c in ms:
        assert any(r0 <= r < r1 and c0 <= c < c1 and (r - r0 >= 8 or r0 == 0)
                   for r0, r1, c0, c1 in bs), (r, c, bs)
    assert any(b[0] == 0 and b[1] >= 16 and b[2] == 0 for b in bs)
    assert any(b[1] == NX and b[0] <= NX - 16 and b[3] == NY for b in bs)
    if width is None:  # merged: disjoint and in order
        assert all(p[1] < n[0] for p, n in zip(bs, bs[1:]))
        # (24 +- 8 overlaps the first 16 rows: one band)
        assert bs[0][:2] == (0, 32) and len(bs) == 5


def test_bands_merge_and_clip():
    f = _shape(100, 40)
    got = LC.bands(f, [(0, 70, 3), (0, 90, 5), (0, 10, 7)], half=32, edge=64)
    assert got == [(0, 100, 0, 40)]
    f = _shape(1000, 42)  # columns cut to a multiple of 4
    assert LC.bands(f, [(0, 500, 3)], half=4, edge=8) == [(0, 8, 0, 40), (496, 504, 0, 40),
                                                         (992, 1000, 0, 40)]


@pytest.mark.parametrize("name,reached", [("DEEP", 4), ("MID3", 3), ("SQUARE", 2), ("WIDE", 2),
                                          ("CELLS", 3)])
def test_field_sets_reach_their_marks(name, reached):
    f = _shape(*LC.SETS[name])
    ms = LC.marks(f)
    assert [m for m, _, _ in ms] == list(LC.MARKS[:reached])
    for m, r, c in ms:
        assert 32 <= r < f.lx - 32, (name, m, r)  # a whole band of owned rows around it
    assert f.rows * f.pitch * 4 <= (16.3 if name == "DEEP" else 8.2) * 2 ** 30
    if name == "DEEP":
        assert f.pitch == 4352 and -(-f.ly // (256 - 2 * LC.HALO)) == 18 and f.lx > 1 << 19
        assert -(-f.lx // 4) > 65535  # the naive kernel's blocks in y
    if name == "WIDE":  # the marks fall mid-row
        assert all(1000 < c < f.ly - 1000 for _, _, c in ms)
    if name == "CELLS":
        assert f.lx * f.ly > 1 << 31


@pytest.fixture(scope="module")
def full_levels():
    """States 0..12 of the whole small plate, with and without a source."""
    out = {}
    for q in (None, 5):
        u = R.init_grid(NX, NY, "random", SEED)
        src = None if q is None else LC.source_window(NX, NY, q, (0, NX, 0, NY))
        lv = [u]
        for _ in range(12):
            lv.append(R.step_np_fma(lv[-1], 0.1, 0.1) if src is None
                      else R.step_np_fma(lv[-1], 0.1, 0.1, source=src))
        out[q] = lv
    return out


@pytest.mark.parametrize("q", [None, 5])
def test_window_oracle_equals_the_full_plate(full_levels, q):
    a, _ = _plate()
    boxes = LC.bands(a, LC.marks(a, SMALL), half=8, edge=16) \
        + LC.bands(a, LC.marks(a, SMALL), half=8, width=64, edge=16) \
        + [(NX - 5, NX, NY - 8, NY), (0, 3, 0, 4), (100, 101, 200, 204)]
    for box in boxes:
        r0, r1, c0, c1 = box
        for k in (1, 2, 8, 12):
            got = LC.window_oracle(NX, NY, SEED, box, k, 0.1, 0.1, q)
            SC.assert_same_bits(got, full_levels[q][k][r0:r1, c0:c1], f"{box} k={k} q={q}")
    lv = LC.window_levels(NX, NY, SEED, boxes[1], 12, q=q)
    for k in range(13):
        SC.assert_same_bits(lv[k], full_levels[q][k][boxes[1][0]:boxes[1][1], :], f"level {k}")


def test_window_oracle_other_coefficients_and_identity():
    box = (120, 150, 40, 80)
    u = R.init_grid(NX, NY, "random", SEED)
    for _ in range(3):
        u = R.step_np_fma(u, 0.07, 0.21)
    SC.assert_same_bits(LC.window_oracle(NX, NY, SEED, box, 3, 0.07, 0.21), u[120:150, 40:80])
    # The whole-plate identity of the GPU tests: zero coefficients change nothing,
    # and the random plate holds no zero (a kernel that skips a store shows).
    u0 = R.init_grid(NX, NY, "random", SEED)
    SC.assert_same_bits(R.step_np_fma(u0, 0.0, 0.0), u0)
    assert (u0 != 0).all()


def test_mfma_chain_is_the_same_step_in_another_association(full_levels):
    u0, canon = full_levels[None][0], full_levels[None][1]
    got = LC.step_np_mfma(u0)
    for edge in (np.s_[0], np.s_[-1], np.s_[:, 0], np.s_[:, -1]):
        SC.assert_same_bits(got[edge], u0[edge], "ring")
    # Not the same bits, and within the 1.87e-5 that step_np_mfma's docstring
    # reckons for values in [0, 100) with cx = cy = 0.1.
    err = np.abs(got - canon).max()
    assert 0 < err <= 1.87e-5
    SC.assert_same_bits(LC.step_np_mfma(u0, 0.0, 0.0), u0)
    box = (120, 150, 40, 80)
    SC.assert_same_bits(LC.window_levels(NX, NY, SEED, box, 1, step=LC.step_np_mfma)[1],
                        got[120:150, 40:80])


def test_harness_on_the_cpu_ops(full_levels):
    a, b = _plate()
    q = ops.Field(NX, NY, LC.HALO, "cpu")
    g = ops.Geom(nx=NX, ny=NY)
    boxes = LC.bands(a, LC.marks(a, SMALL), half=8, edge=16)
    LC.poison(a, b, boxes, 1, SEED)
    for box in boxes:
        ops.naive_step(a, b, g, box)
    for box in boxes:
        got = b.view(*box).numpy()
        SC.assert_same_bits(got, LC.window_oracle(NX, NY, SEED, box, 1), f"naive {box}")
        SC.assert_same_bits(got, full_levels[None][1][box[0]:box[1], box[2]:box[3]], "full")
    assert LC.untouched(b, boxes) == 0
    LC.poison(a, b, boxes, 1, SEED, q=q, qseed=5, grow_q=0)
    for box in boxes:
        ops.source_step(a, b, q, g, box)
        SC.assert_same_bits(b.view(*box).numpy(), LC.window_oracle(NX, NY, SEED, box, 1, q=5),
                            f"source {box}")
    assert LC.untouched(b, boxes) == 0


@pytest.mark.parametrize("wrap", ["", "xy"])
@pytest.mark.parametrize("order", [0, 1])
def test_refine_rows_equals_refine_np(order, wrap):
    fx, fy = 64, 7
    S = RC.source("signed", -(-NX // fx), -(-NY // fy))
    full = R.refine_np(S, NX, NY, fx, fy, order, wrap)
    f = ops.Field(NX, NY, LC.HALO, "cpu", fill=LC.SENTINEL)
    ops.refine(f, S, fx, fy, order=order, wrap=wrap)
    for r0, r1 in [(0, 16), (120, 140), (63, 65), (NX - 16, NX)]:
        rows = LC.refine_rows(S, NX, NY, fx, fy, order, r0, r1, wrap)
        SC.assert_same_bits(rows, full[r0:r1], f"rows {r0}:{r1}")
        SC.assert_same_bits(f.view(r0, r1, 0, NY).numpy(), rows, f"ops.refine rows {r0}:{r1}")
    assert LC.untouched(f, [(0, NX, 0, NY)]) == 0


@pytest.mark.parametrize("fx,fy", [(8, 8), (100, 100), (16, 600), (1, 1), (7, 64)])
def test_coarse_banded_equals_coarse_np(fx, fy):
    a, _ = _plate()
    boxes = LC.bands(a, LC.marks(a, SMALL), half=8, edge=16)
    plate = np.zeros((NX, NY), np.float32)
    vals = []
    for r0, r1, c0, c1 in boxes:
        assert (c0, c1) == (0, NY)
        v = LC.init_window(NX, NY, SEED, (r0, r1, c0, c1)) - np.float32(40.0)  # both signs
        plate[r0:r1] = v
        vals.append((r0, v))
    a.data.zero_()
    a.set_owned(torch.from_numpy(plate))
    want, dev = R.coarse_np(plate, fx, fy), ops.coarse(a, fx, fy)
    got = LC.coarse_banded(vals, NX, NY, fx, fy)
    assert set(got) == {i for r0, r1, _, _ in boxes for i in range(r0 // fx, -(-r1 // fx))}
    for i in range(want["sum"].shape[0]):
        if i in got:
            s, mn, mx, bound = got[i]
            for w in (want, {k: v.numpy() for k, v in dev.items()}):
                assert np.array_equal(mn, w["min"][i]) and np.array_equal(mx, w["max"][i]), i
                assert (np.abs(s - w["sum"][i]) <= bound).all(), i
        else:
            assert not want["sum"][i].any() and not want["min"][i].any() and not want["max"][i].any()


def test_poison_flags_stray_reads_and_writes():
    a, b = _plate()
    g = ops.Geom(nx=NX, ny=NY)
    boxes = LC.bands(a, LC.marks(a, SMALL), half=8, edge=16)
    # A read outside the light cone: the source grown by 0 instead of 1.
    LC.poison(a, b, boxes, 0, SEED)
    ops.naive_step(a, b, g, boxes[1])
    got = b.view(*boxes[1]).numpy()
    assert np.isnan(got[0, 1:-1]).all() and np.isnan(got[-1, 1:-1]).all()
    assert not np.isnan(got[1:-1]).any()
    # A launch on a box one row and one column too large stores outside it.
    LC.poison(a, b, boxes, 2, SEED)
    r0, r1, c0, c1 = boxes[1]
    ops.naive_step(a, b, g, (r0, r1 + 1, c0, c1))
    assert LC.untouched(b, boxes) == c1 - c0
    # Misplaced writes in a NumPy copy: an owned cell between two bands, a
    # ghost cell, a padding cell, and one inside a band (which does not count).
    LC.poison(a, b, boxes, 1, SEED)
    for box in boxes:
        ops.naive_step(a, b, g, box)
    assert LC.untouched(b, boxes) == 0
    for (r, c), n in [((boxes[1][1] + 1, 7), 1), ((-3, 5), 1), ((NX + 2, b.pitch - b.hy - 1), 1),
                      ((boxes[1][0], 9), 0)]:
        bad = ops.Field(NX, NY, LC.HALO, "cpu")
        arr = b.data.numpy().copy()
        arr[b.hx + r, b.hy + c] = 1.0
        bad.data = torch.from_numpy(arr)
        assert LC.untouched(bad, boxes) == n, (r, c)
    bad.data[0, 0] = float("nan")  # a NaN differs from the sentinel too
    assert LC.untouched(bad, boxes) == 1
    assert LC.count_ne(torch.full((5, 7), LC.SENTINEL), LC.SENTINEL) == 0
    assert LC.same_values(a.data[:3], a.data[:3].clone()) is False  # NaN != NaN
    assert LC.same_values(b.data, b.data.clone())
