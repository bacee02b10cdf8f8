"""The checksum on its own, without a GPU: the host heat::checksum_block
(ops.checksum on CPU fields) against the independent NumPy oracle
reference.checksum_np -- the hash computed from the formula, not from the
engine --, block hashes with offsets adding up to the plate's, global indices
beyond 2^32, and what the hash must notice.  tests/test_gpu_service_kernels.py
repeats every case on the device kernel.  Also the CPU side of ops.copy_boxes."""
import numpy as np
import pytest
import torch

from parallel_heat_amd import ops
from parallel_heat_amd.models import reference as R

from . import service_cases as SC

CPU = torch.device("cpu")


def test_oracle_hash_from_first_principles():
    # checksum_np itself, on two cells worked by hand in Python integers.
    def mix(z):
        z = (z + 0x9E3779B97F4A7C15) & SC.M64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & SC.M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & SC.M64
        return z ^ (z >> 31)
    blk = np.array([[1.5, -2.0]], np.float32)
    bits = [0x3FC00000, 0xC0000000]
    ox, oy, ny = 100000, 131000, 131072
    want = sum(mix(((ox * ny + oy + c) * 0x100000001B3 & SC.M64) ^ bits[c]) for c in range(2))
    got = R.checksum_np(blk, ox, oy, ny)
    assert got["hash"] == want & SC.M64
    assert (got["count"], got["min"], got["max"], got["sum"]) == (2, -2.0, 1.5, -0.5)


@pytest.mark.parametrize("name", SC.CHECKSUM_SETS)
@pytest.mark.parametrize("lx,ly", SC.CHECKSUM_SHAPES)
def test_checksum_host_vs_oracle(lx, ly, name):
    v = SC.checksum_values(name, lx, ly)
    SC.assert_checksum(ops.checksum(SC.field_of(v, CPU)), v, what=f"{name} {lx}x{ly}")


@pytest.mark.parametrize("px,py", [(2, 2), (3, 1)])
def test_checksum_blocks_add_up(px, py):
    SC.check_decomposition(CPU, px, py)


def test_checksum_large_indices():
    SC.check_large_indices(CPU)


def test_checksum_sensitivity():
    SC.check_sensitivity(CPU)


def test_checksum_nan():
    SC.check_nan(CPU)


def test_checksum_default_plate_is_the_block():
    v = SC.checksum_values("signed", 5, 7)
    f = SC.field_of(v, CPU)
    assert ops.checksum(f) == ops.checksum(f, 0, 0, 7)


@pytest.mark.parametrize("k", [1, 3])
def test_copy_boxes_cpu_is_slicing(k):
    lx, ly = 13, 17
    src = ops.Field(lx, ly, k, CPU)
    a = SC.payload_array(src)
    src.data.copy_(torch.from_numpy(a))
    dst = ops.Field(lx, ly, k, CPU)
    b = SC.payload_array(dst, first=a.size)
    dst.data.copy_(torch.from_numpy(b))
    pairs = SC.exchange_boxes(lx, ly, k)
    bufs = [torch.zeros(SC.box_size(s), dtype=torch.float32) for s, _ in pairs]
    ops.copy_boxes(src, [(s, buf) for (s, _), buf in zip(pairs, bufs)], True)
    ops.copy_boxes(dst, [(r, buf) for (_, r), buf in zip(pairs, bufs)], False)
    want = b.copy()
    hx, hy = src.hx, src.hy
    for (s, r) in pairs:
        want[hx + r[0]:hx + r[1], hy + r[2]:hy + r[3]] = \
            a[hx + s[0]:hx + s[1], hy + s[2]:hy + s[3]]
    assert np.array_equal(dst.data.numpy().view(np.int32), want.view(np.int32))
    assert np.array_equal(src.data.numpy().view(np.int32), a.view(np.int32))
    with pytest.raises(ValueError):
        ops.copy_boxes(src, [((0, 1, 0, 1), bufs[0])] * 9, True)
