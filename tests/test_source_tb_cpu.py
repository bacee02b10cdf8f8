"""The fused source pass without a GPU: its entry points and Python bindings,
the built kernels' resources (every instantiation scratch-free), and the
launch planner's invariants, which depend on addresses and shapes alone once a
wave cap is set.

The binding test fails on a library without the fused kernel: its entry points
are missing."""
import os
import re
import sys

import pytest

from parallel_heat_amd import _native, ops

from . import source_tb_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = re.compile(r"source_tb_kernelILi(\d)ELb([01])E")


def test_bindings_and_entry_points():
    lib = _native.lib()
    for name in ("heat_op_source_tb_step", "heat_source_tb_plan", "heat_source_tb_set_max_waves",
                 "heat_source_tb_launches"):
        assert getattr(lib, name, None) is not None, name
        assert name in _native._SIGS, name
    for name in ("source_tb_step", "source_tb_plan", "set_source_tb_max_waves",
                 "source_tb_launches"):
        assert callable(getattr(ops, name)) and name in ops.__all__, name
    assert lib.heat_abi_version() == 9
    n = ops.source_tb_launches()
    assert isinstance(n, int) and n >= 0
    # The depth is checked before anything touches a device.
    f = C.FakeField(8, 8, 64, 1 << 20)
    ops.set_source_tb_max_waves(4)
    try:
        for k in (1, 9):
            with pytest.raises(_native.NativeError, match="depth"):
                ops.source_tb_plan(f, f, f, None, k)
    finally:
        ops.set_source_tb_max_waves(0)
    assert ops.source_tb_launches() == n


def test_every_instantiation_is_scratch_free():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        from kernel_resources import kernels
    finally:
        sys.path.pop(0)
    ks = {KERNEL.search(k["name"]).groups(): k for k in kernels(str(_native.LIB_PATH))
          if KERNEL.search(k["name"])}
    # Depths 2 .. 8, each without and with the residual.
    assert sorted(ks) == [(str(k), r) for k in range(2, 9) for r in "01"], sorted(ks)
    bad = [(key, k["scratch"], k["vgpr_spill"]) for key, k in ks.items()
           if k["scratch"] or k["vgpr_spill"]]
    assert not bad, bad
    # Two waves per SIMD at every depth (the launch is sized for that): at most
    # 256 registers per lane; LDS: the residual's two words alone.
    assert all(k["vgpr"] + k["agpr"] <= 256 for k in ks.values()), ks
    assert all(k["lds"] == (8 if key[1] == "1" else 0) for key, k in ks.items()), ks


@pytest.mark.parametrize("shape", C.PLAN_SHAPES, ids=str)
def test_planner_invariants(shape):
    rows, cols, c0, c1, k = shape
    for cap in (1, 2, 7, 2048):
        for phase in (0, 1, 2, 3):
            p = C.check_plan(rows, cols, c0, c1, k, cap, phase)
            # Whole rounds: chunks are shortened only up to the end of the last
            # round of `cap` waves that the longest chunks begin.
            longest = p["strips"] * -(-rows // p["max_chunk_rows"])
            assert longest <= p["units"] <= -(-longest // cap) * cap or p["units"] == longest, \
                (shape, cap, p)
    # A pitch that is no multiple of 4: dword rows, no alignment lead.
    p = C.check_plan(rows, cols, c0, c1, k, 64, phase=1, pitch=c1 + 17 + (c1 + 17) % 2 + 1)
    assert p["vector_rows"] == 0 and p["align"] == 0, p


def test_plan_of_the_flagship_plates():
    # 8192^2 at depth 8 under the MI355X's launch (256 CUs x 8 waves): 35 strips
    # of 240 stored columns, chunks chosen so that the units fill one round.
    p = C.check_plan(8192, 8192, 0, 8192, 8, 2048)
    assert (p["strips"], p["strip_stride"], p["overlap"]) == (35, 240, 8), p
    assert p["units"] <= 2048 < p["strips"] * (p["chunks"] + 1), p
    assert 2 * 8 / p["chunk_rows"] < 0.125, p    # the ramp's share of the rows streamed
