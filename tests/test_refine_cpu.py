"""Starting from a coarse grid, without a GPU: heat::refine_axis against the
NumPy oracle reference.refine_axis_np, the host twin heat::refine_block against
reference.refine_np, properties of the definition, Solver::refine on the CPU
backend alone and across gloo ranks, both CLIs, the stand-alone self-test
(plain and under ASan/UBSan) and the zero-scratch guardrail of the device
kernels (read from the built library's code objects)."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from parallel_heat_amd import _native, ops
from parallel_heat_amd.models import reference as R
from parallel_heat_amd.utils import io as hio

from . import refine_cases as C

ROOT = str(_native.REPO_DIR)
HEAT = str(_native.CLI_PATH)
PY = [sys.executable, "-m", "parallel_heat_amd"]


def test_axis_example_literally():
    for fn in (ops.refine_axis, R.refine_axis_np):
        i0, i1, w = fn(10, 4, 1, False)
        assert i0.dtype == np.int32 and i1.dtype == np.int32 and w.dtype == np.float32
        assert i0.tolist() == [0, 0, 0, 0, 0, 0, 1, 1, 1, 2]
        assert i1.tolist() == [0, 0, 1, 1, 1, 1, 2, 2, 2, 2]
        want = np.array([0, 0, .125, .375, .625, .875, 1 / 6, .5, 5 / 6, 0]).astype(np.float32)
        assert C.bits(w).tolist() == C.bits(want).tolist()
        i0, i1, w = fn(10, 4, 1, True)
        got = [(int(i0[k]), int(i1[k]), float(w[k])) for k in (0, 1, 9)]
        assert got == [(2, 0, .5), (2, 0, float(np.float32(5 / 6))),
                       (2, 0, float(np.float32(1 / 6)))]
        assert i0[2:9].tolist() == [0, 0, 0, 0, 1, 1, 1]
        assert i1[2:9].tolist() == [1, 1, 1, 1, 2, 2, 2]


@pytest.mark.parametrize("wrap", [False, True], ids=["clamp", "wrap"])
@pytest.mark.parametrize("order", C.ORDERS)
def test_axis_matches_oracle(order, wrap):
    for n in range(1, 41):
        for f in list(range(1, 10)) + [64]:
            got, want = ops.refine_axis(n, f, order, wrap), R.refine_axis_np(n, f, order, wrap)
            for g, w, name in zip(got, want, ("i0", "i1", "w")):
                assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (n, f, name)
            i0, i1, w = got
            cells = -(-n // f)
            assert ((i0 >= 0) & (i0 < cells) & (i1 >= 0) & (i1 < cells)).all(), (n, f)
            assert ((w >= 0) & (w < 1)).all() and (w[i0 == i1] == 0).all(), (n, f)


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_host_twin_matches_oracle(case):
    C.check_case("cpu", case)


@pytest.mark.parametrize("cut", C.BLOCK_CUTS, ids=lambda c: f"{c[0]}x{c[1]}")
def test_blocks_make_the_plate(cut):
    C.check_blocks("cpu", cut)


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_order0_inverts_the_coarse_view(case):
    nx, ny, fx, fy = case
    for kind in ("int", "signed"):
        S = C.source(kind, *C.dims(case))
        for wrap in C.WRAPS:
            C.check_order0_inverts_coarse(C.expected(kind, case, 0, wrap), S, fx, fy)
    f = C.nan_field(nx, ny, "cpu")
    ops.refine(f, C.source("signed", *C.dims(case)), fx, fy, order=0)
    C.check_order0_inverts_coarse(f.owned().numpy(), C.source("signed", *C.dims(case)), fx, fy)


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_order1_stays_within_the_sources_range(case):
    nx, ny, fx, fy = case
    for kind in C.KINDS:
        S = C.source(kind, *C.dims(case))
        assert np.isfinite(S).all() and np.abs(S).max() < 2.0 ** 126
        for wrap in C.WRAPS:
            g = C.expected(kind, case, 1, wrap)
            assert S.min() <= g.min() and g.max() <= S.max(), (case, kind, wrap)


def test_plane_is_reproduced_exactly():
    for nx, ny, fx, fy in [(64, 256, 8, 8), (64, 256, 2, 16), (32, 32, 1, 4)]:
        S = C.linear_source(nx, ny, fx, fy)
        C.check_linear_exact(R.refine_np(S, nx, ny, fx, fy, 1), nx, ny, fx, fy)
        f = C.nan_field(nx, ny, "cpu")
        ops.refine(f, S, fx, fy, order=1)
        C.check_linear_exact(f.owned().numpy(), nx, ny, fx, fy)


def test_order0_copies_nan_payloads_and_infinities():
    case = (37, 53, 4, 8)
    nx, ny, fx, fy = case
    S = np.array(C.source("signed", *C.dims(case)))
    u = S.view(np.uint32)
    u[0, 0], u[3, 2], u[9, 6] = 0x7FC12345, 0xFFA00001, 0x7F800001   # quiet, negative, signalling
    S[1, 1], S[2, 5] = np.inf, -np.inf
    want = S[np.arange(nx)[:, None] // fx, np.arange(ny)[None, :] // fy]
    C.assert_bitwise(R.refine_np(S, nx, ny, fx, fy, 0), want, "oracle")
    f = C.nan_field(nx, ny, "cpu")
    ops.refine(f, S, fx, fy, order=0)
    C.assert_bitwise(f.owned().numpy(), want, "host twin")


@pytest.mark.parametrize("wrap", C.WRAPS, ids=lambda w: w or "clamp")
def test_order1_nan_footprint(wrap):
    case = (37, 53, 4, 8)
    nx, ny, fx, fy = case
    for spot in [(0, 0), (4, 3), (9, 6)]:
        S = np.array(C.source("int", *C.dims(case)))
        S[spot] = np.nan
        want = C.nan_footprint(case, wrap, spot)
        assert want.any() and not want.all()
        clean = C.expected("int", case, 1, wrap)
        for name in ("oracle", "host twin"):
            if name == "oracle":
                g = R.refine_np(S, nx, ny, fx, fy, 1, wrap)
            else:
                f = C.nan_field(nx, ny, "cpu")
                ops.refine(f, S, fx, fy, order=1, wrap=wrap)
                g = f.owned().numpy()
            assert np.array_equal(np.isnan(g), want), (name, spot, wrap)
            assert np.array_equal(C.bits(g)[~want], C.bits(clean)[~want]), (name, spot, wrap)


def test_refusals():
    f = C.nan_field(37, 53, "cpu")
    S = C.source("int", 10, 7)
    with pytest.raises(_native.NativeError, match=r"10x7.*5x8.*37x53.*8x7"):
        ops.refine(f, S, 5, 8)
    with pytest.raises(_native.NativeError, match="order"):
        ops.refine(f, S, 4, 8, order=2)
    with pytest.raises(_native.NativeError, match=">= 1"):
        ops.refine(f, S, 0, 8)
    with pytest.raises(ValueError):
        ops.refine(f, S, 4, 8, wrap="z")
    C.assert_frame_intact(f)
    assert _native.lib().heat_abi_version() == 9 == _native.ABI_VERSION
    # A library older than the package lacks an entry point: a clear error, no AttributeError.
    with pytest.raises(_native.NativeError, match="no entry point heat_op_refine_of_tomorrow"):
        _native.call("heat_op_refine_of_tomorrow", 0)


@pytest.mark.parametrize("order", C.ORDERS)
@pytest.mark.parametrize("edges", C.EDGES, ids=C.EDGE_IDS)
def test_cpu_solver_refine_then_steps(edges, order):
    C.check_solver("cpu", edges, order=order, infer=order == 1)


@pytest.mark.parametrize("world,kw", [(4, dict(px=2, py=2)), (3, dict(px=3, py=1))],
                         ids=["2x2", "3x1"])
def test_gloo_ranks_fill_their_own_blocks(tmp_path, world, kw):
    case = C.SOLVER_CASE
    nx, ny, fx, fy = case
    S = C.source("signed", *C.dims(case))
    cfg = dict(nx=nx, ny=ny, steps=0, init="zero", backend="cpu", periodic="xy", **kw)
    res = C.run_world(world, cfg, S, fx, fy, 1, 25, tmp_path)
    assert (int(res["px"]), int(res["py"])) == (kw["px"], kw["py"])
    lv = C.solver_levels(case, 1, "", "xy")
    C.assert_bitwise(res["g0"], lv[0], f"{world} ranks, refined")
    C.assert_bitwise(res["g1"], lv[25], f"{world} ranks, 25 steps")


def _run(cmd, cwd, check=True):
    return subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=300, check=check,
                          env=dict(os.environ, PYTHONPATH=ROOT))


PLATE = ["--backend", "cpu", "--nx", "70", "--ny", "519"]


@pytest.fixture(scope="module")
def view(tmp_path_factory):
    """A coarse view (18 x 65) written by the native CLI from a small run."""
    d = tmp_path_factory.mktemp("view")
    _run([HEAT] + PLATE + ["--steps", "24", "--init", "random", "--seed", "5", "--out", "none",
                           "--out-format", "bin", "--coarse", "4x8", "--coarse-out", "v.bin"], d)
    return str(d / "v.bin")


@pytest.mark.parametrize("extra,order", [([], 1), (["--refine-order", "0", "--refine", "4x8"], 0),
                                         (["--periodic", "y", "--warmup", "3"], 1)],
                         ids=["inferred", "order0", "periodic-warmup"])
def test_both_clis_start_from_the_view(tmp_path, view, extra, order):
    outs = {}
    for name, cmd in (("native", [HEAT]), ("python", PY)):
        d = tmp_path / name
        d.mkdir()
        p = _run(cmd + PLATE + ["--steps", "5", "--init-from", view, "--dump-initial",
                                "--out-format", "bin", "--out", "final.bin", "--json"] + extra, d)
        m = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
        assert m["init_from"] == {"path": view, "rows": 18, "cols": 65, "fx": 4, "fy": 8,
                                  "order": order}
        assert m["steps_done"] == 5
        outs[name] = {f.name: f.read_bytes() for f in sorted(d.iterdir())}
    assert sorted(outs["native"]) == sorted(outs["python"]) == ["final.bin", "initial.dat"]
    for k, v in outs["native"].items():
        assert v == outs["python"][k], k
    S, _ = hio.read_bin(view, mmap=False)
    periodic = "y" if "--periodic" in extra else ""
    g = R.refine_np(S, 70, 519, 4, 8, order, periodic)
    first, h0 = hio.read_bin(str(tmp_path / "native" / "initial.dat"), mmap=False)
    assert h0["step"] == 0
    C.assert_bitwise(first, g, "--dump-initial")
    for _ in range(5):
        g = R.step_np_fma(g, 0.1, 0.1, "", periodic)
    last, h1 = hio.read_bin(str(tmp_path / "native" / "final.bin"), mmap=False)
    assert h1["step"] == 5
    C.assert_bitwise(last, g, "after 5 steps")


@pytest.mark.parametrize("cmd", [[HEAT], PY], ids=["native", "python"])
def test_cli_refuses_bad_init_from(tmp_path, view, cmd):
    base = cmd + PLATE + ["--steps", "1", "--out", "none"]
    p = _run(base + ["--init-from", view, "--refine", "5x8"], tmp_path, check=False)
    assert p.returncode != 0, p.stdout
    for number in ("18x65", "5x8", "70x519", "14x65"):
        assert number in p.stderr, p.stderr
    # Inferred factors that cannot give the file's grid: ceil(200 / 18) = 12, ceil(200 / 12) = 17.
    p = _run(cmd + ["--backend", "cpu", "--nx", "200", "--ny", "519", "--steps", "1", "--out",
                    "none", "--init-from", view], tmp_path, check=False)
    assert p.returncode != 0 and "18x65" in p.stderr and "12x8" in p.stderr and \
        "200x519" in p.stderr and "17x65" in p.stderr, p.stderr
    p = _run(base + ["--init-from", view, "--resume", view], tmp_path, check=False)
    assert p.returncode != 0 and "--init-from" in p.stderr and "--resume" in p.stderr and \
        "choose one" in p.stderr, p.stderr
    p = _run(base + ["--refine", "4x8"], tmp_path, check=False)
    assert p.returncode != 0 and "--refine needs --init-from" in p.stderr, p.stderr
    p = _run(base + ["--init-from", str(tmp_path / "missing.bin")], tmp_path, check=False)
    assert p.returncode != 0 and "missing.bin" in p.stderr, p.stderr


@pytest.mark.parametrize("target", ["refine-selftest", "refine-selftest-asan"])
def test_standalone_selftest(target):
    # The host code alone in a program of its own; nothing loaded into Python
    # runs under a sanitizer.
    p = subprocess.run(["make", "-s", "-C", ROOT, target], capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "refine selftest: ok" in p.stdout


def test_refine_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    lib = os.path.join(ROOT, "parallel_heat_amd", "_lib", "libheat.so")
    if not os.path.exists(lib):
        pytest.skip("libheat.so not built")
    from kernel_resources import kernels
    try:
        ks = kernels(lib)
    except (OSError, Exception) as e:  # noqa: BLE001 - toolchain missing
        pytest.skip(f"cannot read code objects: {e}")
    assert not [k["name"] for k in ks if re.search(r"refine", k["name"])
                and re.search(r"coarse", k["name"])]
    ks = [k for k in ks if re.search(r"refine", k["name"])]
    assert len(ks) >= 1, [k["name"] for k in ks]
    bad = [(k["name"], k["scratch"], k.get("lds", 0)) for k in ks
           if k["scratch"] > 0 or k.get("vgpr_spill", 0) > 0 or k.get("lds", 0) > 0]
    assert not bad, "refine kernels use scratch or LDS: %r" % bad
